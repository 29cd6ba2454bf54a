"""Shared by tests/test_batch_estimate_host.py, tests/test_batch_estimate_gpu.py and tests/golden/make_batch_estimate_golden.py: the
captures of the segmentation's geometry cases and the sessions of the estimate, built once from seeds and fixed patterns.

Geometry: a capture is a pattern of above-noise and below-noise samples (magnitude 1 against 0 with a threshold of 0.5, unless the case is
about the values themselves).  The batch step is S = 64 samples and the reference's outlier_tolerance is 10: the cases put runs of 9 and of
10 samples before, on and behind the seams between steps.  Every case is a capture of its own; all cases of a sample type also form ONE
batch, in the order given, so every capture has neighbours."""
import json
import os

import numpy as np

import noise_cases as nc
from conftest import ROOT, synth_fsk

S = 64
TOL = 10
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "batch_estimate")
RANGES = os.path.join(GOLDEN_DIR, "ranges.npz")
ESTIMATES = os.path.join(GOLDEN_DIR, "estimates.json")

_cache = {}


def from_flags(flags, dtype=np.float32, hi=(1.0, 0.0), lo=(0.0, 0.0)):
    flags = np.asarray(flags, dtype=bool)
    iq = np.where(flags[:, None], np.asarray(hi, dtype=np.float64)[None, :], np.asarray(lo, dtype=np.float64)[None, :]).astype(dtype)
    return np.ascontiguousarray(iq.reshape(-1, 2))


def _pattern(*runs):
    """runs: (above?, length) pairs"""
    return np.concatenate([np.full(n, bool(a)) for a, n in runs]) if runs else np.zeros(0, bool)


def _geometry_f32():
    cases = []
    add = lambda name, flags, thr=0.5: cases.append((name, from_flags(flags), thr))      # noqa: E731
    for n in (0, 1, 9, 10, 11, 19, 20, 21, S - 1, S, S + 1, 3 * S + 9):
        add(f"len{n}-above", np.ones(n, bool))
        add(f"len{n}-below", np.zeros(n, bool))
    add("burst-at-0", _pattern((1, 40), (0, 40)))
    add("burst-after-9", _pattern((0, 9), (1, 50), (0, 30)))
    add("burst-after-10", _pattern((0, 10), (1, 50), (0, 30)))
    n = 4 * S + 20
    for d in (9, 10):
        for off in (0, 30, S - 10, S - 9, S - 5, S - 1, S):
            dip = np.ones(n, bool)
            dip[S + off:S + off + d] = False
            add(f"dip{d}-at{off}", dip)
            add(f"spike{d}-at{off}", ~dip)
    for t in (0, 1, 9, 10):
        add(f"ends-above-then-{t}-below", _pattern((1, 100), (0, t)))
    add("opens-in-the-last-10", _pattern((0, 100), (1, 12)))
    add("opens-at-the-last-sample", _pattern((0, 100), (1, 10)))
    add("opens-short-of-the-end", _pattern((0, 100), (1, 9)))
    # neighbours: the first ends above the noise, the second starts above it -- then the same pair with the second starting below
    add("pair1-ends-above", _pattern((0, 30), (1, 70)))
    add("pair1-starts-above", _pattern((1, 50), (0, 50)))
    add("pair2-ends-above", _pattern((0, 30), (1, 70)))
    add("pair2-starts-below", _pattern((0, 5), (1, 45), (0, 50)))
    # magnitudes equal to the threshold exactly: (3, 4) at 5.0 is NOT above (a strict >); (6, 8) is
    eq = _pattern((0, 20), (1, 60), (0, 20), (1, 30))
    cases.append(("equal-threshold", from_flags(eq, np.float32, hi=(6.0, 8.0), lo=(3.0, 4.0)), 5.0))
    # NaN and infinite samples at lanes 0 and 63: a NaN magnitude is never above, an infinite one is
    odd = from_flags(np.ones(3 * S, bool))
    odd[0] = (np.nan, 0.0)
    odd[S - 1] = (0.0, np.nan)
    odd[S] = (np.inf, 0.0)
    odd[2 * S - 1] = (0.0, -np.inf)
    cases.append(("nan-inf-samples", odd, 0.5))
    quiet = from_flags(np.zeros(3 * S, bool))
    quiet[0] = (np.inf, 0.0)
    quiet[S - 1] = (np.nan, np.nan)
    quiet[2 * S:2 * S + 12] = (np.inf, np.inf)
    cases.append(("inf-spikes-in-noise", quiet, 0.5))
    cases.append(("nan-threshold", from_flags(_pattern((0, 20), (1, 60), (0, 20))), float("nan")))
    # thresholds 40 dB apart between neighbours: the same capture, once with the threshold above its noise and once above its bursts' half
    loud = nc.capture(7001, 4000, "FSK", 1, np.float32, 0.003, 0.5)
    cases.append(("gain-low-threshold", loud, 0.02))
    cases.append(("gain-high-threshold", loud, 2.0))
    cases.append(("gain-tiny-threshold", loud, 0.0002))
    return cases


def _geometry_int(dtype):
    cases = []
    eq = _pattern((0, 20), (1, 60), (0, 20), (1, 30))
    cases.append(("equal-threshold", from_flags(eq, dtype, hi=(6, 8), lo=(3, 4)), 5.0))
    cases.append(("burst-after-10", from_flags(_pattern((0, 10), (1, 50), (0, 30)), dtype, hi=(100, 0)), 50.0))
    if np.dtype(dtype) == np.int16:
        # full scale: (-32768)^2 + (-32768)^2 wraps to -2^31 in C int arithmetic: the magnitude is NaN and never above
        full = from_flags(_pattern((1, 40), (0, 30), (1, 40), (0, 30)), dtype, hi=(20000, 0))
        full[10:25] = (-32768, -32768)
        full[80:82] = (-32768, -32768)
        cases.append(("full-scale-wraps", full, 100.0))
    cases.append(("seeded", nc.capture(7002, 3000, "FSK", 1, dtype, 0.01, 0.5), 8.0 if np.dtype(dtype) == np.int8 else 2000.0))
    return cases


def geometry(dtype=np.float32):
    """[(name, iq, threshold)] of a sample type, in the order of their batch"""
    key = ("geometry", np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = _geometry_f32() if np.dtype(dtype) == np.float32 else _geometry_int(dtype)
        for _, iq, _ in _cache[key]:
            iq.setflags(write=False)
    return _cache[key]


GEOMETRY_DTYPES = (np.float32, np.int8, np.int16)


def many():
    """300 captures of 0 to 40 samples and one of 20 000: the directory scan over more captures than its threads, the compaction's stride"""
    if "many" not in _cache:
        rng = np.random.default_rng(7003)
        caps = [from_flags(rng.random(int(n)) < 0.8) for n in rng.integers(0, 41, 300)]
        caps.insert(150, from_flags(np.repeat(rng.random(400) < 0.5, 50)))
        _cache["many"] = (caps, 0.5)
    return _cache["many"]


# ---- the estimate's sessions -----------------------------------------------------------------------------------------------------
def _golden_iq(name):
    return np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["iq"])


def ook_capture(n_pulses=150, sps=20, seed=7004):
    """an on-off keyed capture of more than 100 pulses, in two messages"""
    rng = np.random.default_rng(seed)
    parts = [np.zeros(300)]
    for m in range(2):
        for _ in range(n_pulses // 2):
            parts += [np.ones(sps * int(rng.integers(1, 3))), np.zeros(sps * int(rng.integers(1, 3)))]
        parts.append(np.zeros(1500))
    env = np.concatenate(parts)
    z = 0.5 * env * np.exp(0.3j) + 0.004 * (rng.standard_normal(len(env)) + 1j * rng.standard_normal(len(env)))
    return np.stack([z.real, z.imag], axis=1).astype(np.float32)


def sps_capture(sps, seed, n=12000):
    """an FSK capture of `sps` samples per symbol: three messages between silent stretches"""
    iq = synth_fsk(n, sps=sps, seed=seed, noise=0.01, pause_every=3000, pause_len=1000)
    iq[:500] = (0.01 * np.random.default_rng(seed + 1).standard_normal((500, 2))).astype(np.float32)
    return np.ascontiguousarray(iq)


def sessions():
    """name -> {"captures": [...], "noise": None / float / list, "modulation": None / str / list}; the captures of a session share
    nothing but their sample type"""
    if "sessions" in _cache:
        return _cache["sessions"]
    out = {}
    gold = [_golden_iq(n) for n in ("ask_short", "fsk", "ask", "fsk4", "steckdose", "enocean_ask", "fsk_sps8")]      # (the longest not first)
    out["goldens-detect"] = dict(captures=gold, noise=None, modulation=None)
    out["goldens-given"] = dict(captures=gold, noise=[0.0299, 0.0011, 0.0175, 0.0, 0.06, 0.0077, 0.0],
                                modulation=["ASK", "FSK", "OOK", "FSK", "FSK", "ASK", "FSK"])
    for mod in ("ASK", "OOK", "FSK"):
        caps = [nc.capture(7100 + i, n, "ASK" if mod == "OOK" else mod, 1, np.float32, sigma, amp)
                for i, ((sigma, amp), n) in enumerate(zip(nc.STREAM_GAINS, nc.N_STREAM))]
        out[f"gains-{mod}"] = dict(captures=caps, noise=None, modulation=mod)
    rng = np.random.default_rng(7005)
    noise_only = (0.01 * rng.standard_normal((5000, 2))).astype(np.float32)
    one_message = np.ascontiguousarray(sps_capture(50, 7202, 6000)[:2900])
    mixed = [sps_capture(20, 7200), noise_only, sps_capture(50, 7201), one_message, ook_capture(), sps_capture(100, 7203),
             np.zeros((0, 2), np.float32), np.zeros((3, 2), np.float32)]
    out["mixed-detect"] = dict(captures=mixed, noise=None, modulation=None)
    out["mixed-shared-noise"] = dict(captures=mixed, noise=0.05, modulation=["FSK", None, "FSK", None, "OOK", None, None, "ASK"])
    out["mixed-noise-per-capture"] = dict(captures=mixed, noise=[0.05, None, 0.06, 0.04, None, 0.05, 0.1, None], modulation=None)
    # a capture for which the reference raises (an infinite sample in every chunk: math.ceil of an infinity) and one whose detected noise is
    # not below the sample type's max_magnitude (the estimate does not ask), between captures it estimates
    bad = np.array(sps_capture(50, 7204, 6000))
    bad[::50, 0] = np.inf
    gates_all = nc.capture(4000, 6000, sigma=1.5, amp=3.0)
    out["raises-detect"] = dict(captures=[sps_capture(20, 7205, 6000), bad, gates_all, sps_capture(100, 7206, 6000)], noise=None, modulation=None)
    for dt in (np.int8, np.int16):
        caps = [nc.capture(7300 + i, n, mod, 1, dt, 0.01, 0.5) for i, (mod, n) in enumerate((("FSK", 20011), ("ASK", 12801), ("FSK", 16384)))]
        out[f"{np.dtype(dt).name}-detect"] = dict(captures=caps, noise=None, modulation=None)
        out[f"{np.dtype(dt).name}-given"] = dict(captures=caps, noise=None, modulation=["FSK", "ASK", "FSK"])
    for s in out.values():
        for c in s["captures"]:
            c.setflags(write=False)
    _cache["sessions"] = out
    return out


def per_capture(value, k):
    return [value] * k if value is None or isinstance(value, (str, float, int)) else list(value)


def load_ranges():
    """name -> int64 (n, 2) of the recorded reference ranges: geometry cases as "<dtype>/<name>", the many-captures batch as "many/<i>\""""
    if "ranges" not in _cache:
        z = np.load(RANGES)
        names, offs, pairs = [str(x) for x in z["names"]], z["offsets"], z["pairs"]
        _cache["ranges"] = {n: pairs[int(offs[i]):int(offs[i + 1])] for i, n in enumerate(names)}
    return _cache["ranges"]


def load_estimates():
    with open(ESTIMATES) as fh:
        return json.load(fh)


def same_estimate(got, want):
    """dict-equal with floats compared by value (an int 0 and a float 0.0 are the same noise)"""
    if got is None or want is None:
        return got is None and want is None
    return set(got) == set(want) and all((got[k] == want[k]) if k == "modulation_type" else (float(got[k]) == float(want[k])) for k in want)
