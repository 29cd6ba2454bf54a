"""A numpy model of k_batch_segments' walk (urh_amd/csrc/batch_estimate.hip; include/urhgpu.h "a batch of captures: message ranges per
capture"): a capture's above-noise flags are taken in steps of 64, each step is a 64-bit mask, and the state machine of
auto_interpretation.segment_messages_from_magnitudes (auto_interpretation.pyx:55-111) is followed over the RUNS of set and clear bits of
that mask, the counters living across the steps' seams.  Written from the kernel's description, step for step, so that the host suite can
hold the walk against the reference without a GPU."""
import numpy as np

STEP = 64
OUTLIER_TOLERANCE = 10


def above_flags(iq, threshold):
    """is sample i above the noise, as the reference compares util.get_magnitudes' value with its `float noise_threshold`: float32 samples
    -- an fp32 square root of the fp32 sum of squares --, integer samples -- C int arithmetic (the sum wraps), a double square root (NaN
    for a negative sum: never above)"""
    iq = np.asarray(iq)
    thr = float(np.float32(threshold))
    with np.errstate(all="ignore"):
        if iq.dtype == np.float32:
            mag = np.sqrt(iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).astype(np.float64)
        else:
            a = iq.astype(np.int64)
            s = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            mag = np.sqrt(s.astype(np.float64))
        return mag > thr


def magnitudes(iq):
    """util.get_magnitudes' values (float32 for float32 samples, float64 otherwise)"""
    iq = np.asarray(iq)
    with np.errstate(all="ignore"):
        if iq.dtype == np.float32:
            return np.sqrt(iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1])
        a = iq.astype(np.int64)
        s = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        return np.sqrt(s.astype(np.float64))


def _ctz(x):
    return (x & -x).bit_length() - 1


def segments(flags):
    """int64 (n, 2) ranges of one capture from its above-noise flags, by the kernel's walk"""
    flags = np.asarray(flags, dtype=bool)
    n = len(flags)
    out = []
    state, conseq_above, conseq_below, start = -1, 0, 0, 0
    full = (1 << STEP) - 1
    for base in range(0, n, STEP):
        cnt = min(STEP, n - base)
        m = 0
        for lane in range(cnt):
            m |= int(flags[base + lane]) << lane
        if base == 0:
            state = 1 if m & 1 else -1
        if state == -1 and m == 0:
            conseq_above = 0
            continue
        if state == 1 and bin(m).count("1") == cnt:
            conseq_below = 0
            continue
        pos = 0
        while pos < cnt:
            bit = (m >> pos) & 1
            other = ((~m & full) if bit else m) >> pos
            run = min(_ctz(other) if other else STEP, cnt - pos)
            at = base + pos
            if state == 1:
                if bit:
                    conseq_below = 0
                elif conseq_below + run >= OUTLIER_TOLERANCE:
                    i_sw = at + (OUTLIER_TOLERANCE - conseq_below) - 1
                    out.append((start, i_sw - OUTLIER_TOLERANCE))
                    state, conseq_below, conseq_above = -1, 0, 0
                else:
                    conseq_below += run
            else:
                if not bit:
                    conseq_above = 0
                elif conseq_above + run >= OUTLIER_TOLERANCE:
                    i_sw = at + (OUTLIER_TOLERANCE - conseq_above) - 1
                    state, start, conseq_below, conseq_above = 1, i_sw - OUTLIER_TOLERANCE, 0, 0
                else:
                    conseq_above += run
            pos += run
    if n > 0 and state == 1 and start < n - conseq_below:
        out.append((start, n - conseq_below))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def capacity(n):
    """urhgpu_batch_segments_capacity: a segment needs ten samples to open and ten to close"""
    return n // (2 * OUTLIER_TOLERANCE) + 1
