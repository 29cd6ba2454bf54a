"""Shared by the tests of a batch with an automatic center per capture (test_batch_center_host.py, test_batch_center_gpu.py) and by
tests/golden/make_batch_center_golden.py: the gain sweep -- captures whose noise floors and amplitudes differ by up to 20 dB, so that no
single center slices them all --, the geometry sweep -- lengths at the edges of the walk's step (64), a leaf (128), a tile (4096), a
pairwise piece (8192) and trims that leave 0 or 1 sample --, the special batches, the oracle's reference for a capture that detects its
own threshold and center, and which outcome the device has to REPORT for it (center_cases.expected: numpy alone)."""
import json
import os
from dataclasses import replace

import numpy as np

import center_cases as cc
import noise_cases as nc
from conftest import synth_fsk

GAIN_MODS = ("ASK", "FSK")
GAIN_DTYPES = (np.float32, np.int16, np.int8)
GAIN_MAX_SIZES = (None, 1000)
GEOMETRY_LENGTHS = (0, 1, 2, 3, 20, 21, 41, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 8193, 12289, 20000)
TINY_KS = (255, 256, 257, 513)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_center", "batch_center.json")
# the 256 outcomes per (modulation, sample type) -- 128 captures at max_size None and 1000 -- with center_cases.expected on the oracle's
# demodulated signals: {class: count}
GAIN_CLASSES = {
    ("ASK", "float32"): {"ok": 233, "none": 20, "tie": 3}, ("ASK", "int16"): {"ok": 229, "none": 19, "tie": 7, "wide": 1},
    ("ASK", "int8"): {"ok": 234, "none": 20, "tie": 2},
    ("FSK", "float32"): {"ok": 150, "tie": 106}, ("FSK", "int16"): {"ok": 152, "tie": 104}, ("FSK", "int8"): {"ok": 191, "tie": 65},
}

_ref = {}


def gain_sweep(mod, dtype):
    """the 128 captures of a (modulation, sample type): eight gains x four seeds x four lengths"""
    out = []
    for i, (sigma, amp) in enumerate(nc.STREAM_GAINS):
        for seed in range(4):
            for n in (nc.N_STREAM[i], 3000, 4097, 1033):
                out.append(nc.capture(7000 + 10 * i + seed, n, mod, 1, np.dtype(dtype), sigma, amp))
    return out


def gain_params(mod):
    return nc.params(mod, 1, write_pos=False)


def geometry_capture(n, dtype):
    """center_cases.capture's recipe at any length (seeded by the length; the gaps are gated for float32 and the signed types)"""
    return synth_fsk(n, sps=cc.SPS, seed=n, noise=0.05, pause_every=2500, pause_len=700, dtype=dtype)


def geometry_sweep(dtype):
    """the 20 lengths, a clean capture first and last (twins)"""
    clean = geometry_capture(3000, dtype)
    return [clean] + [geometry_capture(n, dtype) for n in GEOMETRY_LENGTHS] + [clean]


def geometry_params(mod, dtype):
    return cc.params(mod, dtype, write_pos=False)


def first_sample_batch():
    """clean FSK captures where only sample 0 is filtered (no noise, no gaps: the chain's speculation holds) beside captures with gated gaps"""
    clean = [synth_fsk(n, sps=cc.SPS, seed=50 + n, noise=0.0) for n in (4097, 8193, 300)]
    gaps = [geometry_capture(n, np.float32) for n in (4097, 12289)]
    return [clean[0], gaps[0], clean[1], gaps[1], clean[2], clean[0]]


def noise_between_batch():
    """a capture that is all noise between two good ones"""
    good = nc.capture(7500, 6000, "FSK", 1, np.float32, 0.01, 0.5)
    rng = np.random.default_rng(77)
    noise = (0.01 * rng.standard_normal((5000, 2))).astype(np.float32)
    return [good, noise, good]


def seam_batch():
    """ASK captures at amplitude 0.05 directly beside captures at 0.5: one sample read across a seam moves a center"""
    caps = []
    for j in range(3):
        caps.append(nc.capture(7600 + j, 3000 + 64 * j, "ASK", 1, np.float32, 0.003, 0.05))
        caps.append(nc.capture(7610 + j, 4096 + j, "ASK", 1, np.float32, 0.003, 0.5))
    return caps


def tiny_batch(k):
    """k captures of 0 .. 40 samples out of one pool"""
    rng = np.random.default_rng(k)
    pool = synth_fsk(40_000, sps=8, seed=k, noise=0.08, pause_every=333, pause_len=41)
    lengths, at = rng.integers(0, 41, k), rng.integers(0, 39_000, k)
    return [np.ascontiguousarray(pool[a:a + n]) for a, n in zip(at, lengths)]


def tiny_params():
    from urh_amd.pipeline import DemodParams
    return DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 8, 0.1, 8, False)


def reference(oracle, iq, p, max_size, auto_noise=True, key=None):
    """(noise threshold or None, noise flag, (center or None, qad, pulse table, bits, msg_off, pauses, pos, pos_off)) of the oracle for a
    capture that detects its own threshold (auto_noise) and center; the threshold is not below max_magnitude (flag 2): the slicing of
    zeros(2) with p.center, no center; the reference raises (flag 0): no results.  Computed once per key, left unchanged."""
    full = (key, p.modulation_type, p.bits_per_symbol, max_size, auto_noise)
    if key is not None and full in _ref:
        return _ref[full]
    thr, flag = (None, 1)
    if auto_noise:
        thr, flag = nc.oracle_threshold(oracle, iq)
    if flag == 1:
        ref = cc.reference(oracle, iq, p if thr is None else replace(p, noise_threshold=thr), max_size)
    elif flag == 2:
        qad = np.zeros(2, np.float32)
        assert oracle.detect_center(qad, max_size) is None
        pp, flat = nc.slice_qad(oracle, qad, replace(p, write_bit_sample_pos=True))
        ref = (None, qad, pp) + tuple(flat)
    else:
        ref = None
    out = (thr, flag, ref)
    if key is not None:
        _ref[full] = out
    return out


def expected_class(ref, max_size, pool_bins=cc.POOL_BINS):
    """the class the device has to report for a reference(): center_cases.expected on its demodulated signal"""
    return cc.expected(ref[2][1], max_size, pool_bins)


def bits_hash(bit_strings, pauses):
    """sha256 (12 hex digits) over the messages' bits, as strings of 0 / 1, and their pauses: the golden file's per-capture hash"""
    import hashlib
    return hashlib.sha256(("|".join(bit_strings) + "#" + ",".join(str(int(x)) for x in pauses)).encode()).hexdigest()[:12]


def ref_hash(ref):
    """bits_hash of a reference()"""
    return bits_hash(*nc.messages_of(ref[2][3:6]))


def load_golden():
    with open(GOLDEN) as fh:
        return json.load(fh)
