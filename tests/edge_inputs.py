"""Builders of the edge-value inputs (tests/test_edge_values_host.py, tests/test_edge_values.py, tests/golden/make_edge_golden.py):
captures whose SAMPLE VALUES sit where the demodulation kernels choose between their forms -- non-finite and extreme floats inside
otherwise healthy batches, amplitudes at the fast division's window, samples exactly on the noise gate -- and demodulated signals with
NaN / inf / threshold-equal values for the pulse table.  Everything is seeded and deterministic; float32 captures lie on a 2^-12 grid
(what a converted 13-bit capture looks like), so that a last-bit difference between two hosts' cos / sin cannot change them."""
import zlib

import numpy as np

SPS = 50                                   # samples per symbol of the FSK / ASK captures (PSK: 100, as tests/test_costas_shard.py)
PSK_SPS = 100
N_DEFAULT = 8192 * 4 + 1032                # four hot-kernel chunks and a partial tile
N_PSK = 4096 * 6 + 3                       # beyond 2 * 4096 Costas chunks: the speculative path; two samples in a seventh chunk
N_TIE = 8192 * 2 + 1032
SCALE_K = (-76, -64, -21, -20, -19, 19, 20, 21, 63, 64)
VARIANTS = (0, 1, 2)
DTYPES = (np.float32, np.int8, np.uint8, np.int16, np.uint16)


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


SPECIALS = {
    "nan": _f32(0x7FC00000), "-nan": _f32(0xFFC00000), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf),
    "+3e38": np.float32(3e38), "-3e38": np.float32(-3e38),            # products overflow
    "+1e-30": np.float32(1e-30), "-1e-30": np.float32(-1e-30),        # squares underflow to zero
    "+1e-40": np.float32(1e-40), "-1e-40": np.float32(-1e-40),        # denormal
    "+0": np.float32(0.0), "-0": np.float32(-0.0),
}
NONFINITE = ("nan", "-nan", "+inf", "-inf")
FINITE = tuple(k for k in SPECIALS if k not in NONFINITE)


def same_bits(a, b):
    """elementwise: the same bit pattern, or NaN on both sides"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def both_nan_share(a, b):
    return float((np.isnan(a) & np.isnan(b)).mean())


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _grid(x):
    return (np.round(np.asarray(x, np.float64) * 4096.0) / 4096.0).astype(np.float32)


def _to_dtype(x, dtype):
    """unit-amplitude float64 capture -> dtype at 70 % of full scale (unsigned: around mid-scale); returns (iq, scale)"""
    if np.dtype(dtype) == np.float32:
        return _grid(x), 1.0
    info = np.iinfo(dtype)
    scale, off = (info.max - info.min) / 2 * 0.7, (info.max + info.min + 1) / 2
    return np.clip(np.round(x * scale + off), info.min, info.max).astype(dtype), scale


def _max_magnitude(dtype):
    return {"int8": np.sqrt(127 * 127 + 128 * 128), "uint8": 255.0, "int16": np.sqrt(32768.0 ** 2 + 32767.0 ** 2), "uint16": 65535.0,
            "float32": np.sqrt(2.0)}[np.dtype(dtype).name]


ASK_LEVELS = {2: (0.25, 1.0), 4: (0.25, 0.5, 0.75, 1.0)}


def slicing(mod, dtype=np.float32, order=2, deviation_hz=20e3):
    """(center, center_spacing) that slice base_capture(mod, dtype, order=order) between its levels"""
    if mod == "FSK":
        return 0.0, (2 * np.pi * deviation_hz / 1e6) * 2 / 3 if order == 4 else 1.0
    if mod == "PSK":
        return 0.0, 1.5 if order == 4 else 1.0
    if np.dtype(dtype).kind == "u":                       # raw unsigned values, squared uncentred: the levels ride on the offset
        return float(np.sqrt(2.0) * 0.5 * (np.iinfo(dtype).max + 1) / _max_magnitude(dtype)), 0.1
    unit = 0.9 * (1.0 if np.dtype(dtype) == np.float32 else 0.7 * (np.iinfo(dtype).max - np.iinfo(dtype).min) / 2) / _max_magnitude(dtype)
    lv = ASK_LEVELS[order]
    return float(unit * (lv[0] + lv[-1]) / 2), float(unit * (lv[1] - lv[0]))


def base_capture(mod, dtype=np.float32, n=None, order=2, deviation_hz=20e3, seed=1):
    """A clean FSK / ASK / PSK capture with mild noise and one gated pause; returns (iq, noise_threshold).
    FSK: continuous phase, +-deviation_hz at 1 MS/s (20 kHz: 0.126 rad per sample, the fast loop; 140 kHz: 0.88 rad, the wide loop);
    float32 captures have the amplitude at which the conjugate product's real part is about 1, so that scaled(iq, +-20) puts it at
    2^+-40 with the noise deciding the side.  ASK: a tone with two / four envelope levels.  PSK: the seeded generator of
    tests/test_costas_shard.py with a carrier offset of 0.004 cycles per sample.  Unsigned captures are gated at 0 (the reference
    squares the raw values)."""
    rng = np.random.default_rng([seed, order, int(deviation_hz)])
    if mod == "PSK":
        from test_costas_shard import psk_capture
        n = N_PSK if n is None else n
        a = (n * 11 // 20) // 8 * 8
        iq, noise = psk_capture(n, order, seed=seed + order, dtype=np.dtype(dtype).type, gaps=((a, a + 600),), offset=0.004)
        return (_grid(iq), noise) if np.dtype(dtype) == np.float32 else (iq, noise)
    n = N_DEFAULT if n is None else n
    sym = rng.integers(0, order, n // SPS + 1)
    if mod == "FSK":
        step = 2 * np.pi * deviation_hz / 1e6
        f = np.repeat((2 * sym / (order - 1) - 1) * step, SPS)[:n]
        ph = np.cumsum(f)
        amp = np.full(n, 1.0 / np.sqrt(np.cos(step)) if np.dtype(dtype) == np.float32 else 1.0)
    elif mod == "ASK":
        ph = 2 * np.pi * 0.011 * np.arange(n)
        amp = 0.9 * np.repeat(np.array(ASK_LEVELS[order])[sym], SPS)[:n]
    else:
        raise ValueError(mod)
    x = np.stack([amp * np.cos(ph), amp * np.sin(ph)], 1) + 0.03 * rng.standard_normal((n, 2))
    a = (n // 2) // 8 * 8
    x[a:a + 700] *= 0.01
    iq, scale = _to_dtype(x, dtype)
    return iq, (0.0 if np.dtype(dtype).kind == "u" else 0.2 * scale)


def POSITIONS(n, psk=False):
    """Clusters of neighbouring sample indices where a special goes -- one member of every cluster per capture, so that the specials
    of one capture are at least 300 samples apart and every special sits in a batch that is otherwise in the fast window:
    samples 0 / 1 / 2 and n - 1; a tile seam (2047 / 2048); a chunk seam (8191 / 8192 / 8193); lanes 0 and 63 of a 128-sample row
    (128 r, 128 r + 1 and 128 r + 126, 128 r + 127, every fifth row); for PSK the Costas chunk seams (4095 / 4096 / 4097 and the last
    one, n - 3 .. n - 1 at the default length) and one sample inside the look-back in front of the fourth chunk."""
    fixed = [(0, 1, 2), (2047, 2048), (8191, 8192, 8193), (n - 3, n - 2, n - 1) if psk else (n - 1,)]
    if psk:
        fixed += [(4095, 4096, 4097), (3 * 4096 + 1 - 200,)]
    fixed = [c for c in fixed if 0 <= c[0] and c[-1] < n]
    out = list(fixed)
    for k, r in enumerate(range(3, n // 128, 5)):
        c = (128 * r, 128 * r + 1) if k % 2 == 0 else (128 * r + 126, 128 * r + 127)
        if all(c[0] - f[-1] >= 300 or f[0] - c[-1] >= 300 for f in fixed):
            out.append(c)
    out.sort()
    assert all(b[0] - a[-1] >= 300 for a, b in zip(out, out[1:])), out
    return out


def sprinkle(iq, positions, values):
    """copy of the float32 capture with sample positions[i] overwritten by values[i] = (re, im); None keeps a component"""
    out = np.array(iq, dtype=np.float32, copy=True)
    for pos, (re, im) in zip(positions, values):
        if re is not None:
            out[pos, 0] = re
        if im is not None:
            out[pos, 1] = im
    return out


def sprinkle_plan(n, variant, psk=False):
    """[(position, special's name, component mode)]: mode 0 = the real part, 1 = the imaginary part, 2 = both.
    PSK: an un-gated NaN poisons the loop for the rest of the capture (in the reference too), so NaN / inf go to the last tenth only,
    and +-3e38 -- whose rotated product may be inf - inf -- into one component only; the finite specials take the earlier positions."""
    names = list(SPECIALS)
    plan = []
    chosen = [c[variant % len(c)] for c in POSITIONS(n, psk)]
    late = [p for p in chosen if p >= n - n // 10]
    for i, pos in enumerate(chosen):
        mode = (i // len(names) + i + variant) % 3
        if not psk:
            plan.append((pos, names[(i + 5 * variant) % len(names)], mode))
        elif pos in late:
            plan.append((pos, NONFINITE[(late.index(pos) + variant) % 4], mode))
        else:
            name = FINITE[(i + 3 * variant) % len(FINITE)]
            plan.append((pos, name, mode % 2 if "3e38" in name else mode))
    return plan


def apply_plan(iq, plan):
    vals = [((SPECIALS[name] if mode in (0, 2) else None), (SPECIALS[name] if mode in (1, 2) else None)) for _, name, mode in plan]
    return sprinkle(iq, [p for p, _, _ in plan], vals)


def sprinkled(mod, variant=0, order=2, deviation_hz=20e3, n=None):
    """base_capture(mod, float32) with one special per POSITIONS cluster; returns (iq, noise_threshold, plan).
    Conditions (asserted on the oracle's output): positions where the output is NaN are at most 2 % of an FSK / ASK capture (one bad
    sample costs at most two outputs) and at most 15 % of a PSK capture."""
    iq, noise = base_capture(mod, np.float32, n, order, deviation_hz)
    plan = sprinkle_plan(len(iq), variant, mod == "PSK")
    return apply_plan(iq, plan), noise, plan


def psk_nan_in_gap(order=2, n=None):
    """the PSK capture with a second gated stretch in its last tenth and ONE NaN component in the middle of it: the gate must not fire
    there (NaN <= x is false), so the loop is poisoned from that sample on -- and no earlier.  Returns (iq, noise_threshold, position)."""
    from test_costas_shard import psk_capture
    n = N_PSK if n is None else n
    a, b = (n * 11 // 20) // 8 * 8, n - n // 10 + 100
    iq, noise = psk_capture(n, order, seed=1 + order, gaps=((a, a + 600), (b, b + 500)), offset=0.004)
    iq = _grid(iq)
    iq[b + 250, 0] = SPECIALS["nan"]
    return iq, noise, b + 250


def scaled(iq, k):
    """the float32 capture times 2^k (exact).  k = +-20 puts the conjugate product's real part at 2^+-40, the bounds of the fast
    division's window: between 5 % and 95 % of the products lie inside.  k = -76: the squares underflow, |s|^2 == 0 (0 <= 0: NOISE);
    k = 64: the products overflow."""
    assert iq.dtype == np.float32
    return iq * np.float32(2.0 ** k)


def scaled_threshold(x, k):
    """a noise threshold / center / spacing of the base capture for scaled(iq, k)"""
    return float(np.float32(x) * np.float32(2.0 ** k))


def inside_window_share(iq):
    """share of the conjugate products whose real part lies in [2^-40, 2^40), in float32 as the reference computes it"""
    with np.errstate(all="ignore"):
        re = iq[:-1, 0] * iq[1:, 0] + iq[:-1, 1] * iq[1:, 1]
    return float(((re >= np.float32(2.0 ** -40)) & (re < np.float32(2.0 ** 40))).mean())


# ---- captures on the noise gate -------------------------------------------------------------------------------------------------------
def gate_classes(iq, noise_threshold):
    """-1 / 0 / +1 per sample: c*c + d*d below / equal to / above noise_sqrd in float32 arithmetic, as the reference computes it
    (signal_functions.pyx:293, 366-367: the samples converted to float, products and sum rounded to float32)"""
    c, d = iq[:, 0].astype(np.float32), iq[:, 1].astype(np.float32)
    nt = np.float32(noise_threshold)
    with np.errstate(all="ignore"):
        m, ns = c * c + d * d, nt * nt
    return np.where(m == ns, 0, np.where(m > ns, 1, -1)).astype(np.int8)


def exact_gate_classes(iq, noise_threshold):
    """the same with exact integer arithmetic (integer captures, integer threshold)"""
    c, d = iq[:, 0].astype(np.int64), iq[:, 1].astype(np.int64)
    m, ns = c * c + d * d, int(noise_threshold) ** 2
    return np.where(m == ns, 0, np.where(m > ns, 1, -1)).astype(np.int8)


_TIE_PATTERN = np.array([0, 1, -1, 0, 1, -1, 0, 0, 0, 0, 0, 0, 1, 1, -1, -1, 0, 2, 2, 0], np.int8)   # 2: "float32 and exact disagree", else a tie


def _lattice_tone(points, classes, n, seed, fold=False):
    """a tone through lattice points: sample i takes, among the points of the class _TIE_PATTERN asks for, the one nearest in angle to
    an FSK phase walk (+-0.2 rad per sample, SPS samples per symbol; fold: a triangle wave inside the first quadrant)"""
    rng = np.random.default_rng(seed)
    ph = np.cumsum(np.repeat(np.where(rng.integers(0, 2, n // SPS + 1) == 1, 0.2, -0.2), SPS)[:n])
    if fold:
        ph = np.abs(((ph / (np.pi / 2)) % 2.0) - 1.0) * (np.pi / 2)
    want = _TIE_PATTERN[np.arange(n) % len(_TIE_PATTERN)]
    ang = np.arctan2(points[:, 1].astype(np.float64), points[:, 0].astype(np.float64))
    out = np.zeros((n, 2), points.dtype)
    for cls in (-1, 0, 1, 2):
        idx = np.nonzero(classes == cls)[0]
        sel = np.nonzero(want == cls)[0]
        if len(idx) == 0:                                  # (no such class in this capture: a tie instead)
            idx = np.nonzero(classes == 0)[0]
        dist = np.abs(np.angle(np.exp(1j * (ph[sel, None] - ang[None, idx]))))
        out[sel] = points[idx[np.argmin(dist, axis=1)]]
    return out


def _ring_points(ties, spread, dtype, lo, hi):
    pts = sorted({(x + a, y + b) for x, y in ties for a in range(-spread, spread + 1) for b in range(-spread, spread + 1)
                  if lo <= x + a <= hi and lo <= y + b <= hi})
    return np.array(pts, dtype=dtype)


def tie_capture(dtype, full_scale=False, n=N_TIE):
    """A tone whose amplitude sits ON the noise gate: ties (c*c + d*d == noise_sqrd: NOISE), just-above and just-below samples
    alternate, with runs of six ties.  Returns (iq, noise_threshold).
    int8 / int16: radius 5, threshold 5.0 -- (+-3, +-4), (+-4, +-3), (+-5, 0), (0, +-5).  int16 with full_scale: threshold 30000,
    (+-18000, +-24000), (+-24000, +-18000) and their neighbours up to +-4: the squares are not exact in float32 there and the ROUNDED sum
    decides the gate (class 2 of the pattern: samples where the float32 sum and the exact integer sum fall on different sides, e.g.
    (18004, 23997): 25 above the gate exactly, on it in float32).
    uint8: raw values (0, 200), (56, 192), (120, 160), ... at threshold 200; uint16: the same times 100 with neighbours +-2.
    float32: the int8 capture divided by 128, threshold 5 / 128 (both squares exact).
    Conditions: at least 100 ties, 100 samples strictly above and 100 strictly below in float32 arithmetic; full scale: at least 20
    samples where float32 and exact arithmetic disagree."""
    dt = np.dtype(dtype)
    if dt == np.float32:
        iq, _ = tie_capture(np.int8, n=n)
        return (iq.astype(np.float32) / np.float32(128.0)), 5.0 / 128.0
    quad = [(0, 5), (3, 4), (4, 3), (5, 0)]
    if dt.kind == "u":
        mul = 40 if dt == np.uint8 else 4000
        ties = [(x * mul, y * mul) for x, y in quad] + [(56 * mul // 40, 192 * mul // 40), (192 * mul // 40, 56 * mul // 40)]
        nt, spread, fold = 5.0 * mul, (3 if dt == np.uint8 else 2), True
    elif full_scale:
        assert dt == np.int16
        ties = [(sx * x * 6000, sy * y * 6000) for x, y in quad[1:3] for sx in (1, -1) for sy in (1, -1)]
        nt, spread, fold = 30000.0, 4, False            # (+4, -3) and (-4, +3): exact sum 25 above, float32 sum ON the gate
    else:
        ties = sorted({(sx * x, sy * y) for x, y in quad for sx in (1, -1) for sy in (1, -1)})
        nt, spread, fold = 5.0, 2, False
    info = np.iinfo(dt)
    pts = _ring_points(ties, spread, dt, info.min, info.max)
    cls = gate_classes(pts, nt).astype(np.int8)
    split = (cls > 0) != (exact_gate_classes(pts, nt) > 0)           # gated by one arithmetic, not by the other
    cls[split] = 2
    return _lattice_tone(pts, cls, n, seed=int(nt) + dt.itemsize, fold=fold), nt


def tie_runs(iq, noise_threshold, min_len=4):
    """[(a, b)]: stretches of at least min_len consecutive ties"""
    t = np.concatenate([[0], (gate_classes(iq, noise_threshold) == 0).astype(np.int8), [0]])
    d = np.diff(t)
    return [(int(a), int(b)) for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]) if b - a >= min_len]


# ---- demodulated signals for the pulse table -------------------------------------------------------------------------------------------
NAN_RUNS = (1, 2, 4, 8, 20)


def rect_levels(mod, order):
    """(levels, center, center_spacing)"""
    if mod == "ASK":
        return ((0.2, 0.8), 0.5, 1.0) if order == 2 else ((0.1, 0.4, 0.7, 1.0), 0.55, 0.3)
    return ((-0.5, 0.5), 0.0, 1.0) if order == 2 else ((-0.9, -0.3, 0.3, 0.9), 0.0, 0.6)


def center_thresholds(center, spacing, order):
    """signal_functions.pyx:380-390 in float32"""
    h = order // 2
    c, s = np.float32(center), np.float32(spacing)
    return np.array([c - np.float32(h - (i + 1)) * s for i in range(h)] + [c + np.float32(i + 1 - h) * s for i in range(h, order - 1)], np.float32)


def rect_with_specials(order, mod="FSK", n=6000, seed=3):
    """A demodulated signal for grab_pulse_lens: two / four levels in symbols of 40 samples with single-sample flips and NOISE stretches
    (3, 30 and 300 samples); on top, 100 samples apart: NaN, +inf and -inf alone and in runs of NAN_RUNS samples (shorter and longer
    than the tolerances 2, 3 and 5), every threshold of get_center_thresholds exactly, alone and in runs of 12, and the floats next above
    and next below NOISE (-4, and 0 for ASK) alone and in runs of 8.  Returns (signal, center, center_spacing).
    Conditions: a NaN run longer than the tolerance and one shorter; at least 20 samples equal to a threshold.  The reference sends
    a NaN to the TOP state (`s <= thresholds[k]` is false for every k), never to state 0."""
    rng = np.random.default_rng([seed, order, len(mod)])
    levels, center, spacing = rect_levels(mod, order)
    noise_val = np.float32(0.0 if mod == "ASK" else -4.0)
    x = np.repeat(np.array(levels, np.float32)[rng.integers(0, len(levels), n // 40 + 1)], 40)[:n].copy()
    flips = rng.random(n) < 0.02
    x[flips] = np.array(levels, np.float32)[rng.integers(0, len(levels), int(flips.sum()))]
    for a, ln in ((n - 1500, 3), (n - 1300, 30), (n - 1000, 300)):
        x[a:a + ln] = noise_val
    items = []
    for v in (SPECIALS["nan"], SPECIALS["+inf"], SPECIALS["-inf"], SPECIALS["-nan"]):
        items += [(v, ln) for ln in NAN_RUNS]
    for t in center_thresholds(center, spacing, order):
        items += [(t, 1), (t, 12), (t, 12)]
    for v in (np.nextafter(noise_val, np.float32(np.inf)), np.nextafter(noise_val, np.float32(-np.inf))):
        items += [(v, 1), (v, 8)]
    assert 100 * (len(items) + 1) < n - 1600
    for k, (v, ln) in enumerate(items):
        x[100 * (k + 1):100 * (k + 1) + ln] = v
    return x, center, spacing


def longest_runs(mask):
    """lengths of the runs of True in mask"""
    t = np.concatenate([[0], np.asarray(mask).astype(np.int8), [0]])
    d = np.diff(t)
    return np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]


# ---- the cases the three users share ----------------------------------------------------------------------------------------------------
def float_cases(mod, order=2, deviation_hz=20e3, ks=SCALE_K, variants=VARIANTS):
    """[(tag, iq, noise_threshold, center, center_spacing)] of the float32 value classes: sprinkled (every variant), scaled (every k),
    and for PSK the NaN inside a gated stretch"""
    center, spacing = slicing(mod, np.float32, order, deviation_hz)
    base, noise = base_capture(mod, np.float32, None, order, deviation_hz)
    out = [("sprinkled%d" % v, sprinkled(mod, v, order, deviation_hz)[0], noise, center, spacing) for v in variants]
    for k in ks:
        lin = mod != "FSK"                                 # ASK / PSK outputs scale with the capture, an FSK angle does not
        out.append(("scaled%+d" % k, scaled(base, k), scaled_threshold(noise, k), scaled_threshold(center, k) if lin else center,
                    scaled_threshold(spacing, k) if lin else spacing))
    if mod == "PSK":
        out.append(("nan_in_gap", psk_nan_in_gap(order)[0], noise, center, spacing))
    return out


def tie_cases(mod, dtype, order=2):
    """[(tag, iq, noise_threshold, center, center_spacing)]: the tie capture(s) of the sample type"""
    kinds = (False, True) if np.dtype(dtype) == np.int16 else (False,)
    out = []
    for fs in kinds:
        iq, nt = tie_capture(dtype, full_scale=fs)
        c = 0.0
        if mod == "ASK":
            c = float(np.float32(nt) / np.float32(_max_magnitude(dtype)))      # the ring's own level: ties are NOISE, the rest straddles it
        out.append(("tie_full" if fs else "tie", iq, nt, c, 0.1 if mod != "PSK" else (1.5 if order == 4 else 1.0)))
    return out


def flatten_messages(data, pauses, bit_sample_pos):
    """the reference's _ppseq_to_bits result (lists of arrays) in the flat form of ppseq_to_bits_flat"""
    bits = np.array([b for m in data for b in m], np.uint8)
    off = np.cumsum([0] + [len(m) for m in data]).astype(np.int64)
    pos = np.array([p for m in bit_sample_pos for p in m], np.int64)
    poff = np.cumsum([0] + [len(m) for m in bit_sample_pos]).astype(np.int64)
    return bits, off, np.array(list(pauses), np.int64), pos, poff


# ---- the subset whose reference outputs are committed (tests/golden/make_edge_golden.py -> tests/golden/edge/edge.npz) ----
GOLDEN_FLOAT_TAGS = ("sprinkled0", "scaled-20", "nan_in_gap")
GOLDEN_TOLERANCES = (1, 5)


def golden_demod_cases():
    """[(name, modulation, order, iq, noise threshold, stored with its input)]"""
    out = []
    for mod in ("FSK", "ASK", "PSK"):
        for tag, iq, noise, _, _ in float_cases(mod, 2, ks=(-20,), variants=(0,)):
            assert tag in GOLDEN_FLOAT_TAGS, tag
            out.append((mod + "/" + tag, mod, 2, iq, noise, False))
        for dtype in (np.int8, np.float32):
            for tag, iq, noise, _, _ in tie_cases(mod, dtype):
                out.append(("%s/%s_%s" % (mod, tag, np.dtype(dtype).name), mod, 2, iq, noise, True))
    return out


def golden_rect_cases():
    """[(name, modulation, bits per symbol, signal, center, spacing, tolerance)]"""
    return [("rect/%s/%d/tol%d" % (mod, bps, tol), mod, bps) + rect_with_specials(2 ** bps, mod) + (tol,)
            for mod in ("FSK", "ASK", "PSK") for bps in (1, 2) for tol in GOLDEN_TOLERANCES]


def tie_segments_capture(dtype, full_scale=False, stretch=300):
    """the samples of tie_capture sorted into stretches for the message segmentation, which compares with `>` (a tie is NOT above the
    noise): ties / above / ties / above / below / above / ties -- three messages, which a `>=` would merge into one.
    Returns (iq, noise_threshold)."""
    iq, nt = tie_capture(dtype, full_scale)
    g = gate_classes(iq, nt) if np.dtype(dtype) == np.float32 else exact_gate_classes(iq, nt)   # (integer magnitudes are exact integers)
    pick = {c: iq[g == c] for c in (-1, 0, 1)}
    assert all(len(v) >= 3 * stretch for v in pick.values())
    order, used, parts = (0, 1, 0, 1, -1, 1, 0), {-1: 0, 0: 0, 1: 0}, []
    for c in order:
        parts.append(pick[c][used[c]:used[c] + stretch])
        used[c] += stretch
    return np.ascontiguousarray(np.concatenate(parts)), nt
