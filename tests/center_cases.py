"""Shared by the automatic-center tests (test_auto_center_host.py, test_auto_center_gpu.py): the sweep of captures, the oracle's
reference for a pass that detects its own center, and -- in numpy alone -- which outcome the device has to REPORT for a case, so that
no case can pass through the host fallback unnoticed.

The chain's geometry: tiles of 4096 samples, leaves of 128, pairwise pieces of 8192, the trim int(0.05 k).  The lengths sit below, at
and above a tile / a piece, the max_size values inside one leaf, inside a piece and across pieces."""
import numpy as np

from conftest import synth_fsk

LENGTHS = (3000, 4095, 4096, 4097, 8191, 8193, 12289, 20000, 70001, 262221)
DTYPES = (np.float32, np.int8, np.uint8, np.int16, np.uint16)
MODS = ("FSK", "ASK")
MAX_SIZES = (None, 7500, 1000, 127)
SPS = 50
POOL_BINS = 4096                      # the library's default "auto_center_max_bins"
FLAG = {"ok": 1, "none": 0, "wide": 2, "tie": 3}

_iq, _qad, _ref = {}, {}, {}


def noise_threshold(dtype):
    """float32: 0.3; signed: 0.3 of the amplitude synth_fsk scales to (the gaps are gated: compaction, the first-sample skip);
    unsigned: 0 (nothing is gated: the clean path)"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return 0.3
    if dtype.kind == "u":
        return 0.0
    info = np.iinfo(dtype)
    return 0.3 * 0.7 * (info.max - info.min) / 2


def capture(n, dtype, deviation_hz=100e3):
    key = (n, np.dtype(dtype).name, deviation_hz)
    if key not in _iq:
        _iq[key] = synth_fsk(n, sps=SPS, seed=n, noise=0.05, pause_every=2500, pause_len=700, dtype=dtype, deviation_hz=deviation_hz)
        _iq[key].setflags(write=False)
    return _iq[key]


def params(mod, dtype, bits_per_symbol=1, center_spacing=1.0, write_pos=True, noise=None):
    from urh_amd.pipeline import DemodParams
    return DemodParams(mod, bits_per_symbol, noise_threshold(dtype) if noise is None else noise, 0.25 if mod == "ASK" else 0.0, center_spacing, 5, SPS, 0.1, 8,
                       write_pos)


def demodulated(oracle, iq, p, key=None):
    """oracle.afp_demod of the capture (PSK: qad[0] = -4.0, which the reference leaves unwritten); cached under `key`"""
    if key is not None and key in _qad:
        return _qad[key]
    order = 1 << p.bits_per_symbol
    if p.modulation_type == "PSK":
        qad = oracle.afp_demod(iq, p.noise_threshold, "PSK", order, p.costas_loop_bandwidth)
        qad[0] = -4.0
    else:
        qad = oracle.afp_demod(iq, p.noise_threshold, p.modulation_type, order)
    qad.setflags(write=False)
    if key is not None:
        _qad[key] = qad
    return qad


def sweep_qad(oracle, n, dtype, mod):
    p = params(mod, dtype)
    return demodulated(oracle, capture(n, dtype), p, key=(n, np.dtype(dtype).name, mod))


def histogram(qad, max_size):
    """(counts, edges) as detect_center builds them (AutoInterpretation.py:226-248), None where it returns None before the peak picking"""
    rect = qad[qad > -4]
    rect = rect[int(0.05 * len(rect)):int(0.95 * len(rect))]
    if max_size is not None and len(rect) > max_size:
        rect = rect[0:max_size]
    if len(rect) == 0:
        return None
    hist_min, hist_max = float(rect.min()), float(rect.max())          # util.minmax returns Python floats: float64 edges
    with np.errstate(all="ignore"):
        hist_step = float(np.var(rect))
        try:
            return np.histogram(rect, bins=np.arange(hist_min, hist_max + hist_step, hist_step))
        except (ZeroDivisionError, ValueError):
            return None


def strict_peaks(y):
    """indices of the bins that are strict maxima over +-(window - 1) bins (bins outside count as 0)"""
    nb = len(y)
    w = max(2, int(0.05 * nb) + 1)
    out = []
    for i in range(nb):
        if y[i] > 0 and all(y[i] > (y[i + d] if i + d < nb else 0) and y[i] > (y[i - d] if i - d >= 0 else 0) for d in range(1, w)):
            out.append(i)
    return out


def expected(qad, max_size, pool_bins=POOL_BINS):
    """'none' | 'wide' | 'tie' | 'ok': what the device has to report for this demodulated signal"""
    h = histogram(qad, max_size)
    if h is None:
        return "none"
    y = h[0]
    if len(y) > pool_bins:
        return "wide"
    peaks = strict_peaks(y)
    if not peaks:
        return "none"
    c = sorted((int(y[i]) for i in peaks), reverse=True)
    if len(c) >= 3 and c[1] == c[2]:
        return "tie"
    return "ok"


def sweep():
    """the 400 cases: (mod, dtype, n, max_size)"""
    return [(mod, dt, n, ms) for mod in MODS for dt in DTYPES for n in LENGTHS for ms in MAX_SIZES]


def reference(oracle, iq, p, max_size, key=None):
    """(center or None, qad, pulse table, bits, msg_off, pauses, pos, pos_off) of the oracle for a pass that detects its own center"""
    if key is not None and (key, max_size) in _ref:
        return _ref[(key, max_size)]
    qad = demodulated(oracle, iq, p, key)
    c = oracle.detect_center(qad, max_size)
    pp = oracle.grab_pulse_lens(qad, p.center if c is None else c, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    ref = (None if c is None else float(c), qad, pp) + tuple(oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold))
    if key is not None:
        _ref[(key, max_size)] = ref
    return ref


def assert_equal(got_center, got_qad, got, ref, what):
    """Equal: the center (or None on both sides), the pulse table, bits, offsets, pauses, positions element for element, qad uint32-equal
    from index 1.  got = (ppseq, bits, msg_off, pauses, pos, pos_off)"""
    c, qad, pp, bits, off, pauses, pos, poff = ref
    assert (got_center is None and c is None) or (got_center is not None and c is not None and float(got_center) == c), (what, got_center, c)
    if got_qad is not None:
        assert got_qad.shape == qad.shape and np.array_equal(got_qad[1:].view(np.uint32), qad[1:].view(np.uint32)), what
    assert np.array_equal(got[0], pp), what
    assert np.array_equal(got[1], bits) and np.array_equal(got[2], off) and np.array_equal(got[3], pauses), what
    assert np.array_equal(got[4], pos) and np.array_equal(got[5], poff), what
