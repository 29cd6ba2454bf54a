"""Builders of the batch's edge inputs (tests/test_batch_edges_host.py, tests/test_batch_edges_gpu.py,
tests/golden/make_batch_edge_golden.py): what DevicePipeline.iq_to_bits_batch (urh_amd/csrc/batch.hip) had never been run on -- edge
VALUES through its own quotient and square root (fp64, rounded once), parameters no batch test used, and plans that truncate or are
malformed.  A case is a Batch: captures that share one set of parameters, edge captures between clean ones.  Everything is seeded and
deterministic and every length is derived from the batch's step S (urh_amd.batch.batch_step()), which the callers pass in."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import edge_inputs as E
from conftest import synth_fsk

TOL, PAUSE = 3, 8                          # the A cases' tolerance and pause threshold (as tests/test_edge_values.py)
SCALE_K = (-76, -74, -72, -70, -66, -64, -62, -20, 20, 63, 64)
DENORMAL_K = (-72, -70, -66, -64)          # more than half of the squared magnitudes are non-zero denormals, the signal survives
INT_DTYPES = (np.int8, np.uint8, np.int16, np.uint16)


def n_small(S):
    return 48 * S + 9


@dataclass
class Batch:
    tag: str
    mod: str
    bps: int
    noise: float
    center: float
    spacing: float
    caps: list                             # [(name, iq)]
    tol: int = TOL
    sps: int = E.SPS
    pt: int = PAUSE
    twins: tuple = ()                      # indices of captures whose results must be identical (the clean capture, first and last)
    info: dict = field(default_factory=dict)

    def params(self):
        from urh_amd.pipeline import DemodParams
        return DemodParams(self.mod, self.bps, self.noise, self.center, self.spacing, self.tol, self.sps, 0.1, self.pt, False)

    def arrays(self):
        return [iq for _, iq in self.caps]


def expected(oracle, iq, b):
    """(qad, pulse table, (bits, msg_off, pauses, positions, position offsets)) of the oracle on the capture alone"""
    with np.errstate(all="ignore"):
        qad = oracle.afp_demod(iq, b.noise, b.mod, 2 ** b.bps)
    pp = np.asarray(oracle.grab_pulse_lens(qad, b.center, b.tol, b.mod, b.sps, b.bps, b.spacing)).reshape(-1, 2)
    return qad, pp, oracle.ppseq_to_bits_flat(pp, b.sps, b.bps, True, b.pt)


def _around(b, dtype=np.float32, n=None, order=2):
    """a batch's captures between the clean base capture (first and last: twins) and a short clean capture of another length"""
    base, _ = E.base_capture(b.mod, dtype, n, order)
    other = synth_fsk(777, sps=b.sps, seed=7, noise=0.05, pause_every=300, pause_len=90, dtype=dtype)
    b.caps = [("clean", base)] + b.caps + [("other", other), ("clean", base)]
    b.twins = (0, len(b.caps) - 1)
    return b


# ---- A1: non-finite and extreme float samples ---------------------------------------------------------------------------------------------
def batch_positions(n, S):
    """Clusters of neighbouring sample indices for the specials of a batch capture, one member per capture (variant v takes member
    v mod len): samples 0 / 1 / 2; the first step seam S - 1 / S / S + 1 (lane 0's predecessor is the step before's lane 63, through
    readlane and DPP); 2 S - 1 / 2 S; every fifth step further in, alternating lanes 0 / 1 and lanes 63 / 62; the last full step's lane 63
    and the first sample of the final partial step; n - 1.  The clusters further in are at least 100 samples from every other cluster
    (one that is not is left out); the seams at the head and the tail lie where the step puts them, at least 8 samples apart."""
    last = (n - 1) // S * S                                # first sample of the final (partial or full) step
    head = [(0, 1, 2), (S - 1, S, S + 1), (2 * S - 1, 2 * S)]
    tail = [(last - 1, last), (n - 1,)] if last - 1 > 2 * S + 100 and n - 1 > last else [(n - 1,)]
    fixed = head + tail
    out, k = list(fixed), 0
    for r in range(3, n // S, 5):
        c = (S * r, S * r + 1) if k % 2 == 0 else (S * r + S - 1, S * r + S - 2)
        lo, hi = min(c), max(c)
        if all(lo - max(f) >= 100 or min(f) - hi >= 100 for f in fixed):
            out.append(c)
            k += 1
    out.sort(key=min)
    assert all(min(b) > max(a) for a, b in zip(out, out[1:])) and max(out[-1]) < n, out
    return out


def batch_plans(n, S, variants=E.VARIANTS):
    """{variant: [(position, special's name, component mode)]} -- one member of every cluster per variant.  The names go round the
    lane-63 positions, the lane-0 positions and the rest separately, and a name's j-th use takes component mode j mod 3, so that over the
    variants every special stands at a lane 63, at a lane 0, and in every component mode (asserted in tests/test_batch_edges_host.py)."""
    names = list(E.SPECIALS)
    clusters = batch_positions(n, S)
    slots = [(v, c[v % len(c)]) for v in variants for c in clusters]
    turn = {63: 0, 0: 0, -1: 0}
    used = {name: 0 for name in names}
    plans = {v: [] for v in variants}
    for v, pos in slots:
        kind = 63 if pos % S == S - 1 else (0 if pos % S == 0 else -1)
        name = names[(turn[kind] + (5 if kind == -1 else 0)) % len(names)]
        turn[kind] += 1
        plans[v].append((pos, name, used[name] % 3))
        used[name] += 1
    return plans


def a1_batch(mod, bps, S):
    """the three sprinkled variants of the clean capture between clean ones"""
    n = n_small(S)
    center, spacing = E.slicing(mod, np.float32, 2 ** bps)
    base, noise = E.base_capture(mod, np.float32, n, 2 ** bps)
    plans = batch_plans(n, S)
    b = Batch("A1/%s/%d" % (mod, bps), mod, bps, noise, center, spacing, [("sprinkled%d" % v, E.apply_plan(base, plans[v])) for v in plans])
    b.info["plans"] = plans
    return _around(b, n=n, order=2 ** bps)


def a1_adjacent(mod, S):
    """capture i ends with a NaN / inf sample and capture i + 1 begins with one: neighbours in the device buffer"""
    n = n_small(S)
    center, spacing = E.slicing(mod, np.float32, 2)
    base, noise = E.base_capture(mod, np.float32, n, 2)
    sp = E.SPECIALS
    ends = [(sp["nan"], sp["nan"]), (sp["+inf"], None), (None, sp["-inf"]), (sp["-nan"], sp["+inf"])]
    caps = []
    for i, n_i in enumerate((n, S, S + 1, 2 * S - 1, n)):
        iq = np.array(base[:n_i], copy=True)
        if i > 0:
            iq = E.sprinkle(iq, [0], [ends[(i - 1) % 4]])
        if i < 4:
            iq = E.sprinkle(iq, [n_i - 1], [ends[(i + 1) % 4]])
        caps.append(("edge%d" % i, iq))
    return _around(Batch("A1/adjacent/" + mod, mod, 1, noise, center, spacing, caps), n=n)


# ---- A2: scales ------------------------------------------------------------------------------------------------------------------------------
def a2_batch(mod, bps, k, S):
    n = n_small(S)
    center, spacing = E.slicing(mod, np.float32, 2 ** bps)
    base, noise = E.base_capture(mod, np.float32, n, 2 ** bps)
    lin = mod != "FSK"                                     # ASK outputs scale with the capture, an FSK angle does not
    b = Batch("A2/%s/%d/scaled%+d" % (mod, bps, k), mod, bps, E.scaled_threshold(noise, k), E.scaled_threshold(center, k) if lin else center,
              E.scaled_threshold(spacing, k) if lin else spacing, [("scaled%+d" % k, E.scaled(base, k))])
    return _around(b, n=n, order=2 ** bps)


def denormal_share(iq):
    """share of c*c + d*d, in float32, that is a non-zero denormal"""
    with np.errstate(all="ignore"):
        m = iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]
    return float(((m > 0) & (m < np.finfo(np.float32).tiny)).mean())


# ---- A3: ties on the noise gate -----------------------------------------------------------------------------------------------------------
def tie_counts(iq, nt):
    g = E.gate_classes(iq, nt)
    return int((g == 0).sum()), int((g > 0).sum()), int((g < 0).sum()), int(((g > 0) != (E.exact_gate_classes(iq, nt) > 0)).sum()) \
        if iq.dtype != np.float32 else 0


def tie_capture_short(dtype, full_scale, S):
    """edge_inputs.tie_capture at 16 S + 9 samples, lengthened by S until it meets the counts of the long one (100 ties, 100 above, 100
    below, 10 runs of ties; at full scale 20 samples on which float32 and exact arithmetic disagree)"""
    n = 16 * S + 9
    while True:
        iq, nt = E.tie_capture(dtype, full_scale, n=n)
        t = tie_counts(iq, nt)
        if min(t[:3]) >= 100 and len(E.tie_runs(iq, nt)) >= 10 and (not full_scale or t[3] >= 20):
            return iq, nt
        n += S
        assert n < 200 * S


def a3_batch(mod, dtype, bps, S):
    kinds = (False, True) if np.dtype(dtype) == np.int16 else (False,)
    caps = []
    for fs in kinds:
        iq, nt = tie_capture_short(dtype, fs, S)
        caps.append(("tie_full" if fs else "tie", iq, nt))
    out = []
    for name, iq, nt in caps:                              # (the two int16 captures have thresholds of their own: a batch each)
        center = float(np.float32(nt) / np.float32(E._max_magnitude(dtype))) if mod == "ASK" else 0.0
        b = Batch("A3/%s/%s/%d/%s" % (mod, np.dtype(dtype).name, bps, name), mod, bps, nt, center, 0.1, [(name, iq)])
        base, _ = E.base_capture(mod, dtype, n_small(S))
        b.caps = [("clean", base)] + b.caps + [("tail", np.ascontiguousarray(iq[:S + 3])), ("clean", base)]
        b.twins = (0, len(b.caps) - 1)
        out.append(b)
    return out


def a3_zero_threshold(mod, S):
    """noise_threshold = 0: a sample whose squares underflow to zero is a tie (0 <= 0: NOISE)"""
    n = n_small(S)
    center, spacing = E.slicing(mod, np.float32, 2)
    base, _ = E.base_capture(mod, np.float32, n)
    sp = E.SPECIALS
    at = [S - 1, S, 500, 900]
    iq = E.sprinkle(base, at, [(sp["+1e-30"], sp["-1e-30"]), (sp["-0"], sp["+0"]), (sp["+1e-30"], sp["-1e-30"]), (sp["+1e-40"], sp["-0"])])
    b = Batch("A3/zero/" + mod, mod, 1, 0.0, center, spacing, [("underflow", iq)])
    b.info["at"] = at
    return _around(b, n=n)


# ---- A4: ends of the integer ranges -------------------------------------------------------------------------------------------------------
def range_values(dtype):
    info = np.iinfo(dtype)
    return sorted({info.min, info.min + 1, -1 if info.min < 0 else 1, 0, 1, info.max - 1, info.max})


def range_grid(dtype, S, seed=4):
    """every pairing of the range's end values as (I, Q), in seeded permutations one after the other, 20 S + 9 samples"""
    v = range_values(dtype)
    pairs = np.array([(a, b) for a in v for b in v], dtype=np.int64)
    n = 20 * S + 9
    rng = np.random.default_rng([seed, np.dtype(dtype).itemsize, int(np.iinfo(dtype).min < 0)])
    idx = np.concatenate([rng.permutation(len(pairs)) for _ in range(n // len(pairs) + 1)])[:n]
    return pairs[idx].astype(dtype)


def a4_batch(mod, dtype, half_gate, S):
    mm = E._max_magnitude(dtype)
    noise = float(np.float32(mm / 2)) if half_gate else 0.0
    center = 1.0 if mod == "ASK" else 0.0                  # (ASK: full scale itself, which the corners of the range exceed)
    b = Batch("A4/%s/%s/%s" % (mod, np.dtype(dtype).name, "half" if half_gate else "zero"), mod, 1, noise, center, 0.1,
              [("grid", range_grid(dtype, S))], tol=1, sps=4)
    return _around(b, dtype=dtype, n=n_small(S))


# ---- A5: values equal to a threshold ------------------------------------------------------------------------------------------------------
def a5_capture(dtype, tol, S, seed=5):
    """runs of (3, 4) -- the value ON the threshold --, (4, 4) -- above -- and (3, 3) -- below --, of lengths either side of the tolerance
    and of whole symbols; float32: the same over 128 (every square and sum exact)"""
    rng = np.random.default_rng(seed)
    kinds = np.array([(3, 4), (4, 4), (3, 3)], np.int64)
    lens = [1, tol - 1, tol, tol + 1, tol + 2, 2 * tol + 1, 10, 17, 40]
    n, parts, last = 30 * S + 9, [], -1
    while sum(len(p) for p in parts) < n:
        k = int(rng.integers(0, 3))
        if k == last:
            k = (k + 1) % 3
        last = k
        parts.append(np.repeat(kinds[k][None, :], max(int(lens[int(rng.integers(0, len(lens)))]), 1), 0))
    iq = np.concatenate(parts)[:n]
    return iq.astype(np.int8) if np.dtype(dtype) == np.int8 else (iq.astype(np.float32) / np.float32(128.0))


def a5_threshold(dtype):
    """the float the reference's ASK branch gives for the sample (3, 4): fl32(fl32(sqrt(25 [/ 16384])) / fl32(max magnitude))"""
    if np.dtype(dtype) == np.int8:
        return np.float32(np.float32(5.0) / np.float32(np.sqrt(32513.0)))
    return np.float32(np.float32(5.0 / 128.0) / np.float32(np.sqrt(2.0)))


def a5_batch(dtype, bps, S, center=None):
    """ASK with the center exactly on the value of (3, 4); bps 2: that is thr[1], the neighbours 0.002 away slice nothing else"""
    c = a5_threshold(dtype) if center is None else np.float32(center)
    b = Batch("A5/%s/%d" % (np.dtype(dtype).name, bps), "ASK", bps, 0.0, float(c), 0.002, [("on_threshold", a5_capture(dtype, TOL, S))], sps=10)
    return _around(b, dtype=dtype, n=n_small(S), order=2 ** bps)


# ---- B: parameters no batch test had used -----------------------------------------------------------------------------------------------------
B1_CASES = [(1, 1.0, -0.5), (1, 1.0, 0.5), (2, 0.1, -0.2), (2, 0.1, -0.05), (2, 0.1, 0.05), (2, 0.1, 0.2)]     # (bps, spacing, center)


def b1_batch(bps, spacing, center, tol):
    """FSK captures of one and two samples (afp_demod returns zeros), noise threshold 0: the first row's state is that of the literal 0.0"""
    rng = np.random.default_rng(11)
    caps = [("len%d_%d" % (n, i), (0.5 + rng.random((n, 2))).astype(np.float32)) for i, n in enumerate((1, 2, 2, 1))]
    caps.insert(2, ("len300", synth_fsk(300, sps=10, seed=3, noise=0.05)))
    return Batch("B1/%d/%g/tol%d" % (bps, center, tol), "FSK", bps, 0.0, center, spacing, caps, tol=tol, sps=10)


def b2_batch(mod, bps, S, seed=12):
    """2^bps envelope levels (ASK) or frequency steps (FSK, continuous phase) at 20 samples per symbol, 30 S + 9 samples: a ramp down from
    the top level in front (min(2^bps, 70) symbols), random symbols behind it, a gated pause longer than pause_threshold symbols and a
    shorter one.  Center and spacing slice between the levels."""
    M, sps, n = 2 ** bps, 20, 30 * S + 9
    rng = np.random.default_rng([seed, bps, len(mod)])
    ramp = np.arange(M - 1, M - 1 - min(M, 70), -1)
    sym = np.concatenate([ramp, rng.integers(0, M, n // sps + 1)])[:n // sps + 1]
    lv = np.repeat(sym, sps)[:n]
    h = M // 2
    if mod == "ASK":
        amp = 0.3 + 0.7 * (lv + 1) / M
        ph = 2 * np.pi * 0.011 * np.arange(n)
        spacing = 0.7 / M / np.sqrt(2.0)
        center = (0.3 + 0.7 * (h + 0.5) / M) / np.sqrt(2.0)
    else:
        spacing = 2 * 1.27 / (M - 1)
        amp = np.ones(n)
        ph = np.cumsum((lv - h + 0.5) * spacing)
        center = 0.0
    x = np.stack([amp * np.cos(ph), amp * np.sin(ph)], 1) + 0.0005 * rng.standard_normal((n, 2))
    a = min(len(ramp) * sps + 40, n - 500)
    x[a:a + (PAUSE + 4) * sps] *= 0.001                     # longer than pause_threshold symbols
    x[a + 300:a + 300 + 3 * sps] *= 0.001                   # shorter
    caps = [("levels", x.astype(np.float32)), ("head", x[:S + 1].astype(np.float32)), ("levels_again", x.astype(np.float32))]
    return Batch("B2/%s/%d" % (mod, bps), mod, bps, 0.1, float(center), float(spacing), caps, tol=2, sps=sps, twins=(0, 2))


def b3_batch(sps):
    caps = [("fsk%d" % i, synth_fsk(n, sps=sps, seed=20 + i, noise=0.1, pause_every=300, pause_len=60)) for i, n in enumerate((2000, 333, 2000))]
    caps[2] = ("fsk0", caps[0][1])
    return Batch("B3/sps%d" % sps, "FSK", 1, 0.1, 0.0, 1.0, caps, tol=0 if sps == 1 else 1, sps=sps, pt=8, twins=(0, 2))


B4_SYMBOLS = (65, 128, 129, 200)


def b4_batch(bps):
    """constant tones of 65, 128 and 129 symbols (sps 8) and a gated pause of 200 symbols that pause_threshold = 0 expands to zeros: rows
    of more than 64 symbols, the lanes' second and third rounds"""
    sps = 8
    f = np.concatenate([np.full(65 * sps, 0.5), np.full(128 * sps, -0.5), np.full(129 * sps, 0.5), np.zeros(200 * sps), np.full(65 * sps, -0.5),
                        np.full(128 * sps, 0.5)])
    ph = np.cumsum(f)
    x = np.stack([np.cos(ph), np.sin(ph)], 1)
    a = (65 + 128 + 129) * sps
    x[a:a + 200 * sps] = 0.0
    iq = x.astype(np.float32)
    caps = [("tones", iq), ("short", np.ascontiguousarray(iq[60 * sps:70 * sps])), ("tones_again", iq)]
    return Batch("B4/%d" % bps, "FSK", bps, 0.1, 0.0, 1.0 if bps == 1 else 0.1, caps, tol=2, sps=sps, pt=0, twins=(0, 2))


def b5_batch(k):
    """k tiny captures of 0 .. 40 samples out of one pool: numbers that straddle the directory scan's 256 threads"""
    rng = np.random.default_rng(k)
    pool = synth_fsk(40_000, sps=8, seed=k, noise=0.08, pause_every=333, pause_len=41)
    lengths, at = rng.integers(0, 41, k), rng.integers(0, 39_000, k)
    caps = [("c%d" % i, np.ascontiguousarray(pool[a:a + n])) for i, (a, n) in enumerate(zip(at, lengths))]
    return Batch("B5/%d" % k, "FSK", 1, 0.1, 0.0, 1.0, caps, tol=2, sps=8)


# ---- C: guards and truncation ---------------------------------------------------------------------------------------------------------------
def c1_batch():
    """a capture of 50 .. 200 rows between a capture of one row and a capture of two"""
    one = np.zeros((400, 2), np.float32)                   # everything gated: one PAUSE row
    ph = np.cumsum(np.full(400, 0.3))
    two = np.stack([np.cos(ph), np.sin(ph)], 1).astype(np.float32)      # sample 0 has no predecessor (NOISE), then one tone
    many = synth_fsk(4500, sps=20, seed=31, noise=0.05, pause_every=600, pause_len=250)
    return Batch("C1", "FSK", 1, 0.1, 0.0, 1.0, [("one_row", one), ("many_rows", many), ("two_rows", two)], tol=2, sps=20)


def blob_bytes(n_rows, n_msg, n_bits):
    """size of a batch capture's compact blob (include/urhgpu.h: header, pauses, msg_off, pos_off, int8 states, packed bits, int32 lengths)"""
    up = lambda x: (x + 15) & ~15          # noqa: E731
    o = 128
    for part in (8 * n_msg, 8 * (n_msg + 1), 8 * (n_msg + 1), n_rows, (n_bits + 7) // 8, 4 * n_rows):
        o = up(o + part)
    return o


def region_bytes(n, rows, sps, bps):
    """a capture's region of the work buffer (include/urhgpu.h; as tests/test_batch_host.py::_region_bytes)"""
    up = lambda x: (x + 15) & ~15          # noqa: E731
    rows = max(int(rows), 0)
    msg = rows // 2 + 1
    return up(8 * rows) + up((n // sps + rows // 2 + 2) * bps) + up(8 * (msg + 1)) + up(8 * msg)


SENTINEL = 0xA5


@dataclass
class RawRun:
    work: np.ndarray                       # the whole work allocation afterwards (uint8)
    blob: np.ndarray                       # the whole blob allocation
    counts: np.ndarray                     # (k, 8)
    dir: np.ndarray                        # (k + 1,)
    qad: np.ndarray                        # the whole qad allocation (uint8 view: sentinel bytes where nothing was written)
    lead: int                              # bytes (work, blob, qad) in front of the pointers the library was given
    iq_lead: int                           # samples in front of the d_iq pointer


def run_raw(ctx, iq_alloc, iq_lead, total, starts, plan, k, cp, work_alloc, work_bytes, blob_alloc, blob_cap, lead):
    """urhgpu_iq_to_bits_batch_dev on buffers this call owns, every one larger than what the library is told: iq_alloc holds iq_lead
    samples in front of d_iq and more than `total` behind it; the work, blob and qad allocations (work_alloc / blob_alloc bytes, a float
    per sample of iq_alloc) are filled with SENTINEL and handed over `lead` bytes (qad: iq_lead floats) inside.  Returns host copies."""
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    assert lead % 16 == 0 and work_bytes + lead <= work_alloc and blob_cap + lead <= blob_alloc and iq_lead + total <= len(iq_alloc)
    dev = torch.device("cuda", 0)
    item = 2 * iq_alloc.dtype.itemsize
    assert (iq_lead * item) % 16 == 0
    d_iq = torch.from_numpy(iq_alloc).to(dev)
    d_meta = torch.from_numpy(np.concatenate([np.asarray(starts, np.int64), np.asarray(plan, np.int64)])).to(dev)
    fill = lambda nbytes: torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=dev)      # noqa: E731
    d_work, d_blob, d_qad = fill(work_alloc), fill(blob_alloc), fill(4 * len(iq_alloc))
    d_counts = torch.full((8 * k,), -1, dtype=torch.int64, device=dev)
    d_dir = torch.full((k + 1,), -1, dtype=torch.int64, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.urhgpu_iq_to_bits_batch_dev(ctx.handle, C.c_void_p(d_iq.data_ptr() + iq_lead * item), total, C.c_void_p(d_meta.data_ptr()),
                                               C.c_void_p(d_meta.data_ptr() + 8 * (k + 1)), k, C.byref(cp), C.c_void_p(d_qad.data_ptr() + 4 * iq_lead),
                                               C.c_void_p(d_work.data_ptr() + lead), work_bytes, C.c_void_p(d_counts.data_ptr()),
                                               C.c_void_p(d_dir.data_ptr()), C.c_void_p(d_blob.data_ptr() + lead), blob_cap))
    torch.cuda.synchronize(dev)
    return RawRun(d_work.cpu().numpy(), d_blob.cpu().numpy(), d_counts.cpu().numpy().reshape(k, 8), d_dir.cpu().numpy(), d_qad.cpu().numpy(),
                  lead, iq_lead)
