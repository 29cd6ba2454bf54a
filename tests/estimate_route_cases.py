"""Shared by tests/test_estimate_routes_host.py, tests/test_estimate_routes_gpu.py and tests/golden/make_estimate_routes_golden.py: captures
that send estimators.estimate_dev and DevicePipeline.estimate_batch down every route around their fast path, built from seeds at test time.

  R1  more segments than message_ranges_dev holds (not OOK)        -> a second urhgpu_message_ranges_dev with cap_seg = n_segments
  R2  more merged OOK bursts than the merged capacity              -> a second call with cap_seg = 1, cap_merged = n_merged
  R3  the OOK merge is "ambiguous"                                 -> segment_messages_dev + the numpy merge
  R4  urhgpu_msg_estimate refuses (more than 4096 messages)        -> urhgpu_msg_center_stats (batches of 4096) + urhgpu_msg_plateau_decisions
  R5  a message with more histogram bins than the pool holds       -> the single-message detect_center_dev
  R6  a message whose second and third peak tie                    -> its histogram fetched, numpy decides
  R7  a first plateau that outlasts the 25 % + 65 536 window       -> ALL messages through urhgpu_msg_plateaus + urhgpu_msg_bit_lengths
  R8  equal counts in a message's divisor histogram                -> numpy orders the histogram
  R9  more pooled messages than batch.MSG_GROUP in a session       -> message_decisions in chunks

A scenario is {"captures", "noise", "modulation", "routes"}; noise and modulation are None, one value or one per capture.  The answers of the
real reference are recorded in tests/golden/estimate_routes.json together with what the reference's own pieces say about every capture's
messages (how many segments and messages, how many of them meet each route's condition): the tests assert the routes from that record and
from the call trace, never from the library's own counts."""
import json
import os

import numpy as np

from batch_estimate_cases import per_capture, same_estimate  # noqa: F401  (the tests take them from here)
from conftest import ROOT

RECORD = os.path.join(ROOT, "tests", "golden", "estimate_routes.json")
MANY_GAP, MANY_SYMBOLS, MANY_SPS = 200, 16, 8
MANY_STRIDE = MANY_GAP + MANY_SYMBOLS * MANY_SPS

_cache = {}


def _noise(rng, n, sigma):
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _fsk(rng, n_sym, sps, dev=0.1, lead=0, change=0.5):
    """continuous-phase 2-FSK at +-dev cycles per sample; lead: samples of the upper tone in front; change: how often a symbol differs from
    the one before it"""
    bits = np.cumsum(rng.random(n_sym) < change) & 1
    f = np.concatenate([np.full(lead, dev), np.repeat(np.where(bits == 1, dev, -dev), sps)])
    return np.exp(2j * np.pi * np.cumsum(f))


def _ask(rng, n_sym, sps, low=0.5):
    bits = rng.integers(0, 2, n_sym)
    bits[0] = 1
    return np.repeat(np.where(bits == 1, 1.0, low), sps) * np.exp(0.3j)


def _place(rng, bursts, gaps, sigma, tail=None, amp=1.0, sigma_in=None):
    """bursts between stretches of noise: gaps[i] samples in front of burst i, `tail` (default gaps[-1]) behind the last; sigma_in[i]: the
    noise on burst i where it is not the floor's"""
    tail = gaps[-1] if tail is None else tail
    n = int(sum(gaps) + sum(len(b) for b in bursts) + tail)
    z = _noise(rng, n, sigma)
    pos = 0
    for i, (g, b) in enumerate(zip(gaps, bursts)):
        pos += int(g)
        if sigma_in is not None and sigma_in[i] is not None:
            z[pos:pos + len(b)] *= sigma_in[i] / sigma
        z[pos:pos + len(b)] += amp * b
        pos += len(b)
    return z


def _f32(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=1).astype(np.float32))


def to_dtype(z, dtype):
    """complex samples of at most 1.0 in magnitude (noise aside) over the whole range of an integer sample type: signed around 0, unsigned
    around the middle of the range"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return _f32(z)
    info = np.iinfo(dtype)
    half = (info.max - info.min) // 2
    mid = (info.max + info.min + 1) // 2
    iq = np.stack([z.real, z.imag], axis=1)
    return np.ascontiguousarray(np.clip(np.round(iq * half * 0.98 + mid), info.min, info.max).astype(dtype))


def many_fsk_z(n_msgs, seed=8100):
    rng = np.random.default_rng(seed)
    return _place(rng, [_fsk(rng, MANY_SYMBOLS, MANY_SPS) for _ in range(n_msgs)], [MANY_GAP] * n_msgs, 0.02)


def many_fsk(n_msgs, seed=8100):
    """n_msgs FSK messages of 16 symbols at 8 samples per symbol, 200 samples of noise in front of each"""
    return _f32(many_fsk_z(n_msgs, seed))


def many_fsk_cut(base, n_msgs):
    """the first n_msgs messages of a many_fsk capture: cut in the middle of the gap behind message n_msgs"""
    return np.ascontiguousarray(base[:n_msgs * MANY_STRIDE + MANY_GAP // 2])


def _long_lead(seed, n_more, more_symbols, more_sps, change):
    rng = np.random.default_rng(seed)
    bursts = [_fsk(rng, 60, 100) for _ in range(2)] + [_fsk(rng, 300, 100, lead=120_000)] + [_fsk(rng, 60, 100) for _ in range(3)]
    bursts += [_fsk(rng, more_symbols, more_sps, change=change) for _ in range(n_more)]
    gaps = [5000] * 6 + [400] * n_more
    return _f32(_place(rng, bursts, gaps, 0.01, tail=5000))


def _flat_tone(seed=8300):
    """an unmodulated tone with almost no noise on it between ordinary messages: its demodulated signal is all but constant, so the
    variance-wide bins of detect_center's histogram number tens of thousands"""
    rng = np.random.default_rng(seed)
    tone = np.exp(2j * np.pi * 0.1 * np.arange(6000))
    bursts = [_fsk(rng, 60, 50), _fsk(rng, 60, 50), tone, _fsk(rng, 60, 50), _fsk(rng, 60, 50)]
    return _f32(_place(rng, bursts, [2000] * 5, 0.01, sigma_in=[None, None, 2e-5, None, None]))


def noisy_capture(mod, seed, n_msgs=6, sigma=0.08):
    """the captures the seed searches for tied-peaks and equal-counts walk over: short noisy messages"""
    rng = np.random.default_rng(seed)
    make = (lambda: _fsk(rng, 40, 25, dev=0.02)) if mod == "FSK" else (lambda: _ask(rng, 40, 25))
    return _f32(_place(rng, [make() for _ in range(n_msgs)], [1500] * n_msgs, sigma * 0.25, sigma_in=[sigma] * n_msgs))


def _tied_many():
    """the third message of the tied FSK capture (its histogram's second and third peak tie) with 750 samples of the noise around it, 1100
    times in a row: more tied messages than _settle_centers fetches histograms for at a time"""
    iq = noisy_capture("FSK", TIED_SEEDS["FSK"])
    return np.ascontiguousarray(np.tile(iq[5750:8250], (TIED_MANY, 1)))


def _ook_bursts(n_bursts, seed=8500):
    rng = np.random.default_rng(seed)
    bursts = []
    for _ in range(n_bursts):
        bits = rng.integers(0, 2, 24)
        bits[0] = bits[-1] = 1
        bursts.append(np.repeat(bits.astype(np.float64), 10) * np.exp(0.3j))
    return _f32(_place(rng, bursts, [600] * n_bursts, 0.01))


# seeds found by tests/golden/make_estimate_routes_golden.py --search (a tie in 5-13 % of noisy captures: the first few seeds hold one)
TIED_SEEDS = {"FSK": 8400, "ASK": 8458}
EQUAL_SEEDS = {"FSK": 8402, "ASK": 8400}
TIED_MANY, TIED_MANY_NOISE = 1100, 0.074
OOK_BURSTS = 400
OOK_MERGED_CAP = 256          # what the test lowers estimators.CAP_MERGED to: the capture's merged bursts exceed it


def _session_pooled(seed=8600):
    """45 captures: 40 of 100 to 125 FSK messages each (more than batch.MSG_GROUP in all, so that the FSK group's pooled messages are decided
    in two chunks; an FSK capture's center is the MEAN over its messages, so a single message cut to the wrong capture shows), three of
    short ASK messages, one of noise alone and an empty one, of mixed lengths.  The shapes are those for which the reference's modulation
    vote names the modulation the capture was made with (it takes FSK messages shorter than these for OOK)."""
    rng = np.random.default_rng(seed)
    caps, mods = [], []
    for i in range(45):
        if i == 17:
            caps.append(_f32(_noise(rng, 4000, 0.02))), mods.append("FSK")
        elif i == 30:
            caps.append(np.zeros((0, 2), np.float32)), mods.append("ASK")
        elif i in (5, 20, 38):
            n_msgs, sps = int(rng.integers(85, 125)), int(rng.choice([8, 10, 12]))
            caps.append(_f32(_place(rng, [_ask(rng, 16, sps) for _ in range(n_msgs)], [int(g) for g in rng.integers(150, 260, n_msgs)], 0.02)))
            mods.append("ASK")
        else:
            n_msgs, dev = int(rng.integers(100, 126)), float(rng.choice([0.04, 0.05, 0.06]))
            caps.append(_f32(_place(rng, [_fsk(rng, 64, 8, dev=dev) for _ in range(n_msgs)], [int(g) for g in rng.integers(150, 260, n_msgs)], 0.02)))
            mods.append("FSK")
    return caps, mods


# thresholds in the sample type's own units.  The reference takes an unsigned sample as it stands: a uint8 noise floor around the middle of
# the range has the magnitude 128 * sqrt(2) = 181, so the threshold lies above that.  For uint16 the reference's magnitude is the root of
# I * I + Q * Q in C int arithmetic, which wraps from 46 341 on: the floor's magnitude is NaN or just below 46 341, and only a threshold
# below the half of the circle that faces the origin leaves messages (at 46 000 the reference finds none and answers None)
UNSIGNED_NOISE = {"uint8": 200.0, "uint16": 10000.0, "int8": 12.5, "int16": 3200.0}


def _unsigned(dtype):
    rng = np.random.default_rng(8700)
    fsk = to_dtype(0.95 * many_fsk_z(300, 8701), dtype)
    ask = to_dtype(0.95 * _place(rng, [_ask(rng, 60, 50) for _ in range(5)], [3000] * 5, 0.02), dtype)
    return [fsk, ask]


def scenarios():
    """name -> {"captures": [...], "noise", "modulation", "routes": the routes the scenario exists for}"""
    if "scenarios" in _cache:
        return _cache["scenarios"]
    out = {}
    base = many_fsk(4200)
    out["many-fsk-4200"] = dict(captures=[base], noise=0.1, modulation="FSK", routes=("R1", "R4"))
    # as many messages as the first urhgpu_message_ranges_dev call and one urhgpu_msg_estimate call hold, and one more
    out["many-fsk-cut-4096"] = dict(captures=[many_fsk_cut(base, 4096)], noise=0.1, modulation="FSK", routes=())
    out["many-fsk-cut-4097"] = dict(captures=[many_fsk_cut(base, 4097)], noise=0.1, modulation="FSK", routes=("R1", "R4"))
    out["many-fsk-8300"] = dict(captures=[many_fsk(8300, 8101)], noise=0.1, modulation="FSK", routes=("R1", "R4"))
    out["long-lead"] = dict(captures=[_long_lead(8200, 0, 0, 0, 0.5)], noise=None, modulation="FSK", routes=("R7",))
    out["long-lead-retry"] = dict(captures=[_long_lead(8201, 800, 400, 8, 0.9)], noise=0.1, modulation="FSK", routes=("R7",))
    out["flat-tone"] = dict(captures=[_flat_tone()], noise=None, modulation="FSK", routes=("R5",))
    for mod in ("FSK", "ASK"):
        out[f"tied-peaks-{mod}"] = dict(captures=[noisy_capture(mod, TIED_SEEDS[mod])], noise=None, modulation=mod, routes=("R6",))
        out[f"equal-counts-{mod}"] = dict(captures=[noisy_capture(mod, EQUAL_SEEDS[mod])], noise=None, modulation=mod, routes=("R8",))
    out["tied-many"] = dict(captures=[_tied_many()], noise=TIED_MANY_NOISE, modulation="FSK", routes=("R6",))
    out["ook-bursts"] = dict(captures=[_ook_bursts(OOK_BURSTS)], noise=0.1, modulation="OOK", routes=("R2", "R3"))
    caps, mods = _session_pooled()
    out["session-pooled"] = dict(captures=caps, noise=0.1, modulation=mods, routes=("R9",))
    out["session-pooled-detect"] = dict(captures=caps, noise=0.1, modulation=None, routes=("R9",))
    for dt in (np.uint8, np.uint16, np.int8, np.int16):
        out[f"unsigned-{np.dtype(dt).name}"] = dict(captures=_unsigned(dt), noise=UNSIGNED_NOISE[np.dtype(dt).name], modulation=["FSK", "ASK"], routes=())
    for s in out.values():
        for c in s["captures"]:
            c.setflags(write=False)
    _cache["scenarios"] = out
    return out


def load_record():
    if "record" not in _cache:
        with open(RECORD) as fh:
            _cache["record"] = json.load(fh)
    return _cache["record"]


def expected(name):
    """the recorded estimates of a scenario's captures (dicts, None where the reference gives None)"""
    return [c["estimate"] for c in load_record()[name]]
