"""Inputs of the tests of the batch's DC correction (tests/test_batch_dc_host.py, tests/test_batch_dc_gpu.py; urh_amd/batch/
dc_correct_batch, iq_to_bits_batch_dc), each built once and read-only.  The expected values are numpy's own expression per capture
(dc_cases.numpy_dc) -- never the code under test."""
import functools
import warnings

import numpy as np

import batch_psk_cases
import dc_cases
from conftest import synth_fsk

DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.float32)

# ---- the length sweep: 70 captures (more than two wavefronts of 32), not sorted by length ---------------------------------------------------
SWEEP_K = 70
SWEEP_FIXED = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8193, 20_001)
FIRST_START, UNUSED_BEHIND = 3, 5


def numpy_dc(x):
    """dc_cases.numpy_dc; an empty capture gives an empty capture and the means NaN (numpy warns about the empty slice)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return dc_cases.numpy_dc(x)


def sentinel(dtype, n):
    """the pattern of the samples that belong to no capture"""
    a = (np.arange(2 * n).reshape(n, 2) * 37 + 11) % 119
    return a.astype(dtype)


def pack(caps, dtype, first=FIRST_START, behind=UNUSED_BEHIND):
    """(iq_cat, starts): the captures back to back from sample `first`, `behind` unused samples behind the last one"""
    lengths = np.array([len(c) for c in caps], np.int64)
    starts = first + np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cat = sentinel(dtype, int(starts[-1]) + behind)
    for c, s in zip(caps, starts[:-1]):
        cat[int(s):int(s) + len(c)] = c
    return cat, starts


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sweep(dtype):
    """(captures, iq_cat, starts, [(numpy's output, numpy's mean)])"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(77)
    lengths = np.concatenate([SWEEP_FIXED, rng.integers(100, 3001, SWEEP_K - len(SWEEP_FIXED))])
    lengths = lengths[rng.permutation(SWEEP_K)]
    assert len(lengths) == SWEEP_K and (np.diff(lengths) < 0).any() and (np.diff(lengths) > 0).any()
    caps = [dc_cases.generic(dtype, int(n), seed=j) for j, n in enumerate(lengths)]
    cat, starts = pack(caps, dtype)
    want = [numpy_dc(c) for c in caps]
    _frozen(cat, starts, *caps, *[a for w in want for a in w])
    return caps, cat, starts, want


# ---- the float32 values: every case of dc_cases.F32_CASES at a length past 3 * CHUNK (the "seam" cases index it), three long ones ---------------
F32_N = 12_301
F32_LONG = (("dc_10x_pos", 100_003), ("zero_mean_spiked", 100_003), ("ties_odd_k", 100_003))


@functools.lru_cache(maxsize=None)
def f32_values():
    """(names, captures, [(numpy's output, numpy's mean)])"""
    assert F32_N > 3 * dc_cases.CHUNK
    names = [(name, F32_N) for name in sorted(dc_cases.F32_CASES)] + list(F32_LONG)
    got = [dc_cases.f32_case(name, n) for name, n in names]
    return [f"{name}:{n}" for name, n in names], [g[0] for g in got], [(g[1], g[2]) for g in got]


@functools.lru_cache(maxsize=None)
def int_values(name):
    """(captures, [(numpy's output, numpy's mean)]) of one of dc_cases.int_cases(): the case, and two stretches of it that start on other
    alignments"""
    x = dc_cases.int_cases()[name]
    caps = [x, np.ascontiguousarray(x[5:7_782]), np.ascontiguousarray(x[1:1_000])]
    want = [numpy_dc(c) for c in caps]
    _frozen(*caps, *[a for w in want for a in w])
    return caps, want


# ---- demodulation sets: six captures each on a DC term ------------------------------------------------------------------------------------------
SET_LENGTHS = (30_011, 12_000, 40_000, 8_193, 25_000, 33_333)
SETS = ("fsk", "ask", "ask_i16_auto_noise_records", "psk")
ASK_SETS = ("ask", "ask_i16_auto_noise_records")


def ask_capture(n, sps, seed, dtype):
    """on a fifth of the time, so that the corrected on and off levels stay apart; the DC term is minus half the on level, so that on and off
    have the same magnitude and slicing goes wrong without the correction -- whatever the noise threshold is, a detected one included"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n // sps + 1)
    env = np.repeat(bits, sps)[:n].astype(np.float64)
    for a in range(20 * sps, n, 70 * sps):
        env[a:a + 50 * sps] = 0
    iq = np.stack([env * 0.8, env * 0.3], axis=1) + 0.01 * rng.standard_normal((n, 2)) + (-0.4, -0.15)
    if np.dtype(dtype) == np.float32:
        return iq.astype(np.float32)
    return np.round(iq * 20_000).astype(dtype)


@functools.lru_cache(maxsize=None)
def demod_set(kind):
    """(captures, DemodParams, sample type, options of iq_to_bits, numpy-corrected captures)"""
    from urh_amd.pipeline import DemodParams
    if kind == "fsk":
        caps = [synth_fsk(n, sps=50, seed=n, noise=0.02, pause_every=3000, pause_len=1500) * np.float32(0.5) + np.array([0.2, 0.1], np.float32)
                for n in SET_LENGTHS]
        out = caps, DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 50, 0.1, 8, True), np.float32, {}
    elif kind == "ask":
        caps = [ask_capture(n, 50, n, np.float32) for n in SET_LENGTHS]
        out = caps, DemodParams("ASK", 1, 0.2, 0.45, 1.0, 2, 50, 0.1, 8, True), np.float32, {}
    elif kind == "ask_i16_auto_noise_records":
        caps = [ask_capture(n, 50, n, np.int16) for n in SET_LENGTHS]
        out = (caps, DemodParams("ASK", 1, 4000.0, 9000.0, 1.0, 2, 50, 0.1, 8, True), np.int16,
               {"auto_noise": True, "msg_records": True, "message_length_divisor": 4})
    else:
        caps = [(batch_psk_cases.psk_capture(n, 2, seed=n)[0] + np.array([0.3, -0.2], np.float32)).astype(np.float32) for n in SET_LENGTHS]
        out = caps, batch_psk_cases.params(2, 0.2), np.float32, {}
    caps = [np.ascontiguousarray(c) for c in out[0]]
    corrected = [numpy_dc(c)[0] for c in caps]
    _frozen(*caps, *corrected)
    return (caps, *out[1:], corrected)


def batch_options(options):
    """the options of iq_to_bits as iq_to_bits_batch_dc takes them"""
    o = {"auto_noise": bool(options.get("auto_noise", False))}
    if options.get("msg_records"):
        o["message_length_divisor"] = options["message_length_divisor"]
    return o


def oracle_bits(oracle, iq, p, options):
    """(pulse table, bits) of the oracle on a capture as it is: the noise threshold detected where the set asks for it"""
    noise = p.noise_threshold
    if options.get("auto_noise"):
        noise = oracle.detect_noise_level(oracle.get_magnitudes(iq))
    qad = oracle.afp_demod(iq, noise, p.modulation_type, 2 ** p.bits_per_symbol, p.costas_loop_bandwidth)
    pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    return np.asarray(pp).reshape(-1, 2), oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)[0]
