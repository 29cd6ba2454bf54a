"""Executable model (numpy, CPU tensors) of the engine methods behind ShardedPipeline.detect_noise_level / detect_center
(urh_amd/shard_engine.py: noise_partials, compact_gt, pairwise_partial, histogram), written from their definitions in
include/urhgpu.h and csrc/pairwise.hpp: the CPU suite drives the orchestration and the record combiner of urh_amd/sharding.py with it
over ThreadComm, and the GPU suite compares the kernels' records with the model's."""
import numpy as np
import torch

from urh_amd import sharding as S


def _np(t):
    return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def magnitudes(iq):
    """util.get_magnitudes (util.pyx:128-136): float32 samples in float32 (sqrtf), integer samples with the products and the sum in a
    wrapping C int and the root in double"""
    iq = _np(iq)
    if iq.dtype == np.float32:
        return np.sqrt(iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).astype(np.float64)
    a = iq.astype(np.int64)
    s32 = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    with np.errstate(invalid="ignore"):
        return np.sqrt(s32.astype(np.float64))


def mapped(x, mode, mean):
    x = np.asarray(x, dtype=np.float32)
    if mode == 0:
        return x
    with np.errstate(all="ignore"):
        d = x - np.float32(mean)
        return d * d


def full_piece_sums(a):
    """pw of every piece of 8192 float32 (a: (P * 8192,)): leaves of 128 = 8 strided accumulators, then the perfect tree over 64 leaves"""
    with np.errstate(all="ignore"):
        r = np.add.accumulate(a.reshape(-1, 64, 16, 8), axis=2, dtype=np.float32)[:, :, -1, :]
        s = ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def partial_record(x, g_off, m_total, mode, mean, words=None):
    """the record of urhgpu_pairwise_partial_f32_dev (include/urhgpu.h) for x = elements [g_off, g_off + len(x)) of m_total"""
    x = np.asarray(x, dtype=np.float32)
    m = len(x)
    g0, g1 = int(g_off), int(g_off) + m
    pa, pb = S.pairwise_inside_pieces(g0, m, m_total)
    n_words = S.PW_REC_PIECES + pb - pa
    rec = np.zeros(n_words if words is None else int(words), np.float32)
    assert len(rec) >= n_words
    rec[0:4] = np.array([g0, m], np.int64).view(np.float32)
    ok = x[~np.isnan(x)]
    rec[4] = ok.min() if len(ok) else np.inf
    rec[5] = ok.max() if len(ok) else -np.inf
    rec[6] = x[0] if m else 0.0
    rec[7:8] = np.array([n_words], np.int32).view(np.float32)
    if m == 0:
        return rec
    a = mapped(x, mode, mean)
    if pb > pa:
        rec[S.PW_REC_PIECES:n_words] = full_piece_sums(a[pa * S.PW_PIECE - g0:pb * S.PW_PIECE - g0])
    p_first, p_last = g0 // S.PW_PIECE, (g1 - 1) // S.PW_PIECE
    for p, area in ((p_first, S.PW_REC_FIRST),) + (((p_last, S.PW_REC_LAST),) if p_last != p_first else ()):
        if pa <= p < pb:
            continue
        for off, ln in S.pairwise_piece_leaves(p, m_total):
            l0, l1 = p * S.PW_PIECE + off, p * S.PW_PIECE + off + ln
            lo, hi = max(l0, g0), min(l1, g1)
            if hi <= lo:
                continue
            if l0 >= g0 and l1 <= g1:
                rec[area + (off + 63) // 64] = S.pairwise_leaf_sum(a[l0 - g0:l1 - g0])
            else:
                dst = S.PW_REC_HEAD if l0 < g0 else S.PW_REC_TAIL
                rec[dst:dst + hi - lo] = a[lo - g0:hi - g0]
    return rec


class ModelEstimatorEngine:
    """the estimator methods of an engine, on numpy arrays / CPU tensors"""

    def noise_partials(self, iq_local, pos_base, n_total, chunk, n_chunks):
        mag = magnitudes(iq_local)
        n_local = len(mag)
        out = np.zeros((2, n_chunks), np.float64)
        for k in range(n_chunks):
            lo, hi = n_total - (k + 1) * chunk, n_total - k * chunk
            a, b = max(lo, pos_base) - pos_base, min(hi, pos_base + n_local) - pos_base
            if b > a:
                out[0, k] = mag[a:b].sum()
                out[1, k] = mag[a:b].max()            # np.max: NaN if any
        return torch.from_numpy(out)

    def compact_gt(self, x, thr):
        x = _np(x)
        if x.dtype != np.float32 or x.ndim != 1:
            raise ValueError("detect_center: a float32 1-D tensor (the shard's demodulated signal)")
        kept = np.zeros(max(len(x), 1), np.float32)
        k = x[x > np.float32(thr)]
        kept[:len(k)] = k
        return torch.from_numpy(kept), torch.tensor([len(k)], dtype=torch.int64)

    def pairwise_partial(self, x, g_off, m_total, mode, mean, words):
        return torch.from_numpy(partial_record(_np(x), g_off, m_total, mode, mean, words))

    def histogram(self, x, edges):
        return torch.from_numpy(np.histogram(_np(x), bins=edges)[0].astype(np.int64))


def cut_lists(rng, n):
    """ways of cutting a sequence of n elements into 1, 2, 3 and 8 parts: at random points, at multiples of 128 and of 8192, and with
    empty parts.  Each a list of (begin, end) in order."""
    out = []
    for parts in (1, 2, 3, 8):
        picks = [sorted(int(c) for c in rng.integers(0, n + 1, parts - 1))]
        picks.append(sorted(int(c) // 128 * 128 for c in rng.integers(0, n + 1, parts - 1)))
        picks.append(sorted(min(n, int(c) // 8192 * 8192) for c in rng.integers(0, n + 8192, parts - 1)))
        if parts > 1:
            c = sorted(int(c) for c in rng.integers(0, n + 1, max(parts - 2, 1)))
            picks.append(sorted((c + c)[:parts - 1]))                       # repeated cut points: empty parts
            picks.append([0] * (parts - 1))                                 # everything on the last rank
            picks.append([n] * (parts - 1))                                 # ... on the first
        for c in picks:
            e = [0] + list(c) + [n]
            out.append([(e[r], e[r + 1]) for r in range(parts)])
    return out


# ---- seeded inputs shared by the CPU and the GPU suite ---------------------------------------------------------------------------
def bounds_for(n, world):
    """shard_bounds where it shards the capture; for captures it refuses (shorter than two samples per rank) plain equal cuts,
    empty shards included"""
    try:
        return S.shard_bounds(n, world)
    except ValueError:
        per = -(-n // world)
        return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(world)]


def bursty_capture(n, seed, dtype=np.float32):
    """noise with bursts of carrier (about a third of the capture): detect_noise_level finds the noise floor's maximum.  Integer
    components stay below 2^15, so that I^2 + Q^2 fits a C int and every magnitude is a number: a uint16 sample with larger components
    has a NaN magnitude (magnitude.hpp), which the tests of that case put in themselves."""
    rng = np.random.default_rng(seed)
    amp = np.where((np.arange(n) // max(1, n // 7)) % 3 == 1, 1.0, 0.02)
    iq = (rng.standard_normal((n, 2)) * 0.5 + 1.0) * amp[:, None]
    if dtype == np.float32:
        return iq.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.round(iq * info.max * 0.4), info.min, min(info.max, 32767)).astype(dtype)


def two_level(n, seed, noise_runs=True):
    """a demodulated signal: two levels with a little noise, and (noise_runs) stretches of -4 of random length, as afp_demod leaves
    them where the capture is below the noise threshold"""
    rng = np.random.default_rng(seed)
    x = (np.where(rng.integers(0, 2, n // 50 + 1).repeat(50)[:n] == 1, 0.8, -0.6) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    if noise_runs:
        at = 0
        while at < n:
            at += int(rng.integers(200, 3000))
            ln = int(rng.integers(1, 1500))
            x[at:at + ln] = -4.0
            at += ln
    return x


COMBINER_LENGTHS = (5, 127, 128, 129, 1023, 8191, 8192, 8193, 16384 + 1, 3 * 8192 + 777, 40_000)


def run_ranks(world, work, timeout=120):
    """work(rank, comm) on `world` threads over ThreadComm -> (results, exceptions); a rank that raises releases the others"""
    import threading
    shared = S.ThreadComm.Shared(world)
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            out[r] = work(r, S.ThreadComm(shared, r))
        except BaseException as e:          # noqa: BLE001 -- reported by the caller
            err[r] = e
            shared.barrier.abort()
    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), "a rank hangs"
    return out, err
