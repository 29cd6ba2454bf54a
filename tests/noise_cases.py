"""Shared by the automatic-noise tests (test_auto_noise_host.py, test_auto_noise_gpu.py) and by tests/golden/make_auto_noise_golden.py:
captures built from seeds, the demodulation parameters that go with them, the list of fixture cases, and the oracle's reference for a
pass that detects its own noise threshold.

The recipe: complex Gaussian noise of sigma per component with bursts of amplitude `amp` (FSK, ASK or PSK symbols of `SPS` samples);
the first tenth and the last tenth of the capture are left silent, and so are the gaps between the three bursts -- detect_noise_level's
quiet chunks.  Integer sample types hold the same capture scaled to the type's range (unsigned: around its mid-point)."""
import json
import os

import numpy as np

SPS = 100
DTYPES5 = (np.float32, np.int8, np.uint8, np.int16, np.uint16)
PASS_DTYPES = (np.float32, np.int16, np.int8)
# (modulation, bits per symbol) of the one-pass tests; "QAM" is a modulation the demodulator leaves at zeros (URHGPU_MOD_OTHER)
PASS_MODS = (("ASK", 1), ("FSK", 1), ("FSK", 2), ("QAM", 1), ("PSK", 1), ("PSK", 2))
N_PASS = 60000
CHAIN_SIZES = (4, 99, 100, 101, 199, 200, 12801, 300007)          # chunk 1 against 2, 199 against 100 chunks, a dropped front remainder
HOST_SIZES = (0, 3, 4, 99, 100, 101, 199, 200, 12801, 60000)
# the stream: noise floors and amplitudes that differ by up to 20 dB (a factor of 10), so that no single threshold decodes them all
STREAM_GAINS = ((0.03, 0.5), (0.003, 0.05), (0.01, 0.5), (0.003, 0.1), (0.03, 0.3), (0.005, 0.05), (0.02, 0.5), (0.003, 0.05))
N_STREAM = (20011, 20000, 16384, 20011, 12801, 20000, 20011, 16384)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "auto_noise.json")

_cache = {}


def scale_to(iq, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return iq.astype(np.float32)
    info = np.iinfo(dtype)
    half = info.max if dtype.kind == "i" else info.max // 2
    off = 0 if dtype.kind == "i" else half + 1
    return np.clip(np.round(iq * half + off), info.min, info.max).astype(dtype)


def capture(seed, n, mod="FSK", bits_per_symbol=1, dtype=np.float32, sigma=0.01, amp=0.5):
    """(n, 2) samples of `dtype`, read-only, cached"""
    key = (seed, n, mod, bits_per_symbol, np.dtype(dtype).name, sigma, amp)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    z = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    lo, hi = n // 10, n - n // 10
    seg = (hi - lo) // 3
    order = 1 << bits_per_symbol
    for b in range(3):
        a0, a1 = lo + b * seg, lo + b * seg + (2 * seg) // 3
        if a1 <= a0:
            continue
        sym = np.repeat(rng.integers(0, order, (a1 - a0) // SPS + 1), SPS)[:a1 - a0]
        if mod == "ASK":
            burst = amp * (sym + 1) / order * np.exp(0.3j)
        elif mod == "PSK":
            burst = amp * np.exp(1j * (2 * np.pi * sym / order + np.pi / order))
        else:                                              # FSK (also what a "QAM" pass is given): continuous phase, +-20 kHz (order 4: +-10 / +-30 kHz) at 1 MS/s
            f = (2 * sym - (order - 1)) * (20e3 if order == 2 else 10e3)
            burst = amp * np.exp(1j * np.cumsum(2 * np.pi * f / 1e6))
        z[a0:a1] += burst
    iq = scale_to(np.stack([z.real, z.imag], axis=1), dtype)
    iq.setflags(write=False)
    _cache[key] = iq
    return iq


def params(mod, bits_per_symbol=1, noise=0.0, write_pos=True):
    """the slicing that goes with capture(): FSK around 0 (order 4: thresholds at 0 and +-0.125 rad per sample), ASK between its two
    levels (0.25 and 0.5 of the amplitude over max_magnitude), PSK around 0"""
    from urh_amd.pipeline import DemodParams
    center = 0.265 if mod == "ASK" else 0.0
    spacing = 0.125 if mod == "FSK" else 1.0
    return DemodParams(mod, bits_per_symbol, noise, center, spacing, 5, SPS, 0.1, 8, write_pos)


def pass_cases():
    """the fixture's cases: name -> keyword arguments of capture()"""
    cases = {}
    for k, (mod, bps) in enumerate(PASS_MODS):
        for j, dt in enumerate(PASS_DTYPES):
            cases[f"pass-{mod}{1 << bps}-{np.dtype(dt).name}"] = dict(seed=1000 + 10 * k + j, n=N_PASS, mod=mod, bits_per_symbol=bps, dtype=np.dtype(dt).name)
    for i, ((sigma, amp), n) in enumerate(zip(STREAM_GAINS, N_STREAM)):
        cases[f"stream-{i}"] = dict(seed=2000 + i, n=n, mod="FSK", bits_per_symbol=1, dtype="float32", sigma=sigma, amp=amp)
    for n in (12801, 300007):
        cases[f"size-{n}"] = dict(seed=3000 + n % 7, n=n, mod="FSK", bits_per_symbol=1, dtype="float32")
    cases["gates-all"] = dict(seed=4000, n=N_PASS, mod="FSK", bits_per_symbol=1, dtype="float32", sigma=1.5, amp=3.0)      # threshold >= sqrt(2): flag 2
    cases["file-float32"] = dict(seed=5000, n=N_PASS, mod="FSK", bits_per_symbol=1, dtype="float32")
    cases["file-int8"] = dict(seed=5001, n=N_PASS, mod="FSK", bits_per_symbol=1, dtype="int8")
    return cases


def case_capture(kw):
    kw = dict(kw)
    kw["dtype"] = np.dtype(kw["dtype"])
    return capture(**kw)


def load_golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def constant_envelope(n=60000, dtype=np.float32):
    """a carrier without gaps: the chunk means lie within 10 % of each other -> detect_noise_level returns 0"""
    ph = 2 * np.pi * 0.01 * np.arange(n)
    return scale_to(0.5 * np.stack([np.cos(ph), np.sin(ph)], axis=1), dtype)


def oracle_threshold(oracle, iq):
    """detect_noise_level(get_magnitudes(iq)) -> (value, flag) by the flag rules of include/urhgpu.h; where it raises: (the exception, 0)"""
    import model_noise
    try:
        value = oracle.detect_noise_level(oracle.get_magnitudes(iq))
    except (ValueError, OverflowError) as exc:
        return exc, 0
    return float(value), (1 if value < model_noise.max_magnitude(iq.dtype) else 2)


def reference(oracle, iq, p, noise, center=None):
    """(qad, pulse table, flat bits) of the oracle's afp_demod -> grab_pulse_lens -> _ppseq_to_bits with the given noise threshold"""
    order = 1 << p.bits_per_symbol
    if p.modulation_type == "PSK":
        qad = oracle.afp_demod(iq, noise, "PSK", order, p.costas_loop_bandwidth)
        qad[0] = -4.0                                      # (the reference leaves result[0] of the Costas loop unwritten; the library documents -4.0)
    else:
        qad = oracle.afp_demod(iq, noise, p.modulation_type, order)
    return (qad,) + slice_qad(oracle, qad, p, center)


def slice_qad(oracle, qad, p, center=None):
    c = p.center if center is None else center
    pp = oracle.grab_pulse_lens(qad, c, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    flat = oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, p.write_bit_sample_pos, p.pause_threshold)
    return pp, flat


def messages_of(flat):
    """(list of bit strings, list of pauses) from ppseq_to_bits_flat's tuple"""
    bits, off, pauses = flat[0], flat[1], flat[2]
    return ["".join(map(str, bits[off[i]:off[i + 1]].tolist())) for i in range(len(pauses))], [int(x) for x in pauses]
