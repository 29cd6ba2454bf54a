"""Executable model (numpy, CPU tensors) of the engine behind ShardedPipeline.iq_to_bits_auto (urh_amd/shard_engine.py: demod_own, demod,
demod_qad, set_center, and runs on the demodulated shard), built from the run-segmentation model (tests/model_shard.py, whose `runs` takes a
demodulated shard) and the estimators' model (tests/model_shard_estimators.py), with afp_demod from the caller (the oracle's).  The CPU suite
drives the orchestration of urh_amd/sharding.py with it over ThreadComm.  Also: the seeded captures the CPU and the GPU suite share.
TEST INFRASTRUCTURE ONLY."""
import dataclasses

import numpy as np
import torch

import model_shard as MS
import model_shard_estimators as ME

SAMPLE_TYPES = (np.float32, np.int8, np.uint8, np.int16, np.uint16)


class ModelAutoEngine(MS.ModelShardEngine, ME.ModelEstimatorEngine):
    """shards are numpy arrays (n_local, 2) of a sample type.  afp_demod(iq, noise, modulation, order) -> float32 (n,)"""

    def __init__(self, afp_demod, pipelined=False, **kw):
        super().__init__(**kw)
        self.afp_demod = afp_demod
        if pipelined:
            self.tail_stream = object()          # what the orchestration takes for a pipelined engine
        self._qad = self._seam = self._center = None
        self.demod_calls = 0

    def tail(self, iq_local, p):
        return torch.from_numpy(np.array(np.asarray(iq_local)[-2:]))

    def demod_own(self, iq_local, left_halo=None):
        if getattr(self, "tail_stream", None) is not None:
            raise ValueError("a pass that demodulates first runs on an engine that is not pipelined")
        iq = np.asarray(iq_local)
        if iq.ndim != 2 or iq.shape[1] != 2:
            raise ValueError("IQ must be an (N, 2) array")
        if iq.dtype not in [np.dtype(t) for t in SAMPLE_TYPES]:
            raise ValueError("Unsupported dtype")
        if not iq.flags.c_contiguous:
            raise ValueError("iq_to_bits_auto: the shard must be contiguous")
        if left_halo is not None and (np.asarray(left_halo).shape != (2, 2) or np.asarray(left_halo).dtype != iq.dtype):
            raise ValueError("left_halo: the two samples before the shard, shape (2, 2)")

    def demod(self, iq_local, left, pos_base, n_total, rank, world, p):
        """afp_demod of halo + shard: output 0 (NOISE: the halo's first sample has no predecessor here) dropped, output 1 is the seam value
        -- the demodulated value of the sample before the shard --, the rest rows [pos_base, pos_base + n_local) of afp_demod(capture)"""
        iq = np.asarray(iq_local)
        order = 1 << p.bits_per_symbol
        if rank == 0:
            self._qad, self._seam = self.afp_demod(iq, p.noise_threshold, p.modulation_type, order), None
        else:
            full = self.afp_demod(np.concatenate([ME._np(left).astype(iq.dtype), iq]), p.noise_threshold, p.modulation_type, order)
            self._qad, self._seam = np.ascontiguousarray(full[2:]), np.float32(full[1])
        self._center = None
        self.demod_calls += 1

    def demod_qad(self):
        return self._qad

    def demod_seam(self):
        return self._seam

    def set_center(self, center):
        self._center = float(center)

    def runs(self, iq_local, left, pos_base, n_total, rank, world, p, want_qad):
        if self._qad is None:                    # the fused pass: demodulation and runs in one
            self.demod(iq_local, left, pos_base, n_total, rank, world, p)
        if self._center is not None:
            p = dataclasses.replace(p, center=self._center)
        q, seam = self._qad, self._seam
        self._qad_out, self._qad, self._center = q, None, None
        return super().runs(q, None if rank == 0 else [seam], pos_base, n_total, rank, world, p, want_qad)

    def bits_finish(self, flags_all):
        piece = super().bits_finish(flags_all)
        piece["qad"] = self._qad_out
        return piece


# ---- seeded captures shared by the CPU and the GPU suite ---------------------------------------------------------------------------
def _to_dtype(iq, dtype):
    """float samples of amplitude about 1 in a sample type: integers scaled to 0.4 of their range (unsigned: around the middle), below 2^15
    so that every magnitude is a number (see model_shard_estimators.bursty_capture)"""
    if np.dtype(dtype) == np.float32:
        return iq.astype(np.float32)
    info = np.iinfo(dtype)
    if np.dtype(dtype).kind == "u":
        hi = min(info.max, 32767)
        return np.clip(np.round(iq * hi * 0.2 + hi * 0.5), 0, hi).astype(dtype)
    return np.clip(np.round(iq * info.max * 0.4), info.min, info.max).astype(dtype)


def message_capture(n, mod, dtype=np.float32, sps=50, seed=0, order=2, burst=None, gap=None, noise=0.02, low=None, blank=None, offset=0.0):
    """bursts of `burst` modulated samples between gaps of `gap` samples of noise alone (the capture begins and ends in a gap; 2300 and 900
    for captures of up to 32 000 samples, in proportion above):
    detect_noise_level finds the gaps' maximum, detect_center the middle between the levels.  ASK: amplitudes 0.5 / 1.0 on a carrier;
    FSK: continuous phase, order 2 +-0.1 cycles per sample, order 4 +-0.05 and +-0.15.
    low = (a, b): the ASK amplitude is 0.5 throughout [a, b); blank = (a, b): those samples are exactly zero (below every gate);
    offset: a constant added to both components (what a DC correction removes)."""
    gap = max(900, n // 40 + 100) if gap is None else gap          # more than two of detect_noise_level's chunks of n // 100: some are quiet
    burst = gap * 5 // 2 + 50 if burst is None else burst
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, order, n // sps + 1)
    t = np.arange(n)
    if mod == "ASK":
        amp = np.repeat(np.where(sym % 2 == 1, 1.0, 0.5), sps)[:n]
        ph = 2 * np.pi * 0.013 * t
    else:
        f = (np.array([-0.1, 0.1]) if order == 2 else np.array([-0.15, -0.05, 0.05, 0.15]))[sym]
        amp = np.ones(n)
        ph = np.cumsum(2 * np.pi * np.repeat(f, sps)[:n])
    if low is not None:
        amp[low[0]:low[1]] = 0.5
    on = ((t - gap) % (burst + gap)) < burst
    on &= t < n - gap // 2
    iq = np.stack([np.cos(ph), np.sin(ph)], 1) * (amp * on)[:, None] + noise * rng.standard_normal((n, 2))
    if blank is not None:
        iq[blank[0]:blank[1]] = 0.0
    return _to_dtype(iq + offset, dtype)


def params(mod, order=2, sps=50, center=None, write_pos=True):
    """parameters whose center and noise threshold are NOT the capture's: a pass that takes them gives other bits than an automatic one"""
    from urh_amd.pipeline import DemodParams
    if center is None:
        center = 0.05 if mod == "ASK" else 0.75
    return DemodParams(mod, 1 if order == 2 else 2, 0.0, center, 0.6 if order == 4 else 1.0, 5, sps, 0.1, 8, write_pos)


def loud_capture(n, seed=0):
    """float32: quiet chunks of magnitude 2.0, bursts of magnitude 30 -- the noise level (2.0) is not below max_magnitude (2 ** 0.5)"""
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, n)
    mag = np.where((np.arange(n) // max(1, n // 7)) % 3 == 1, 30.0, 2.0)
    return (np.stack([np.cos(ph), np.sin(ph)], 1) * mag[:, None]).astype(np.float32)


def reference(oracle, iq, p, center_max_size=None, auto_noise=True, auto_center=True):
    """the chain on the whole capture: detect_noise_level -> afp_demod -> detect_center -> grab_pulse_lens -> ppseq_to_bits_flat.
    Returns dict(noise, center (None: not found), qad, flat = (ppseq, bits, msg_off, pauses, pos, pos_off))"""
    noise = oracle.detect_noise_level(oracle.get_magnitudes(iq)) if auto_noise else p.noise_threshold
    qad = oracle.afp_demod(iq, noise, p.modulation_type, 1 << p.bits_per_symbol)
    c = oracle.detect_center(qad, center_max_size) if auto_center else None
    pp = oracle.grab_pulse_lens(qad, p.center if c is None else c, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    flat = (pp,) + tuple(oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold))
    return dict(noise=noise if auto_noise else None, center=None if c is None else float(c), qad=qad, flat=flat)


def run_ranks_together(world, work, timeout=30):
    """work(rank, comm) on `world` threads over ThreadComm -> (results, exceptions), like model_shard_estimators.run_ranks, but a rank that
    raises does NOT release the others: for cases in which every rank has to raise by itself.  A rank left alone in a collective gets a
    BrokenBarrierError after `timeout` seconds, which the caller sees among the exceptions."""
    import threading
    from urh_amd import sharding as S
    shared = S.ThreadComm.Shared(world)
    shared.barrier = threading.Barrier(world, timeout=timeout)
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            out[r] = work(r, S.ThreadComm(shared, r))
        except BaseException as e:          # noqa: BLE001 -- reported by the caller
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(2 * timeout)
    assert not any(t.is_alive() for t in ts), "a rank hangs"
    return out, err


def assert_flat_equal(got, want, what=""):
    names = ("ppseq", "bits", "msg_off", "pauses", "pos", "pos_off")
    for name, a, b in zip(names, got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (what, name, np.asarray(a).shape, np.asarray(b).shape)
