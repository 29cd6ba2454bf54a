"""A numpy model of the message records a pass ends with (include/urhgpu.h: urhgpu_msg_record) -- the arithmetic the kernel
k_msg_records restates, written from its semantics and independent of urh_amd: the padding decision, the first and the middle
position, and the RSSI as the float64 mean of the window's normalised magnitudes with numpy's pairwise summation order spelled out
(so that the ORDER is what is tested, not np.mean against itself).

numpy's float64 np.add.reduce over a contiguous array walks it in pieces of 8192 elements (the ufunc buffer size), total =
((0 + pw(piece 0)) + pw(piece 1)) + ..., where pw is the pairwise routine:
    n < 8    : 0 + a[0] + a[1] + ...
    n <= 128 : eight accumulators r[j] = a[j]; r[j] += a[i + j] for i = 8, 16, .. < n - n % 8;
               ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the n % 8 tail in order
    n > 128  : n2 = n / 2, n2 -= n2 % 8; pw(a[:n2]) + pw(a[n2:])
(test_msg_records_host.py holds this against np.mean for every length up to 20 000; ONE pairwise tree over the whole array differs
from np.mean at 4172 of the lengths between 8193 and 20 000.)
"""
import numpy as np

LEAF = 128
RECORD_DTYPE = np.dtype([("rssi", "<f8"), ("first_pos", "<i8"), ("mid_pos", "<i8"), ("n_pad", "<i4"), ("flag", "<i4")])


def leaves_of(n):
    """the leaves (offset, length) of the pairwise tree over n terms, in order, and the tree as nested tuples of leaf indices"""
    leaves = []

    def walk(off, ln):
        if ln <= LEAF:
            leaves.append((off, ln))
            return len(leaves) - 1
        n2 = ln // 2
        n2 -= n2 % 8
        return (walk(off, n2), walk(off + n2, ln - n2))
    tree = walk(0, n)
    return leaves, tree


def leaf_sums(a, leaves):
    """the pairwise sum of every leaf: leaves of one length are summed together, eight accumulators each (elementwise float64 adds)"""
    out = np.zeros(len(leaves), np.float64)
    offs = np.array([o for o, _ in leaves], dtype=np.int64)
    lens = np.array([ln for _, ln in leaves], dtype=np.int64)
    for ln in np.unique(lens).tolist():
        sel = np.nonzero(lens == ln)[0]
        block = a[offs[sel][:, None] + np.arange(ln)[None, :]]            # (leaves of this length, ln)
        if ln < 8:
            res = np.zeros(len(sel), np.float64)
            for i in range(ln):
                res = res + block[:, i]
        else:
            lim = ln - ln % 8
            r = block[:, 0:8].copy()
            for i in range(8, lim, 8):
                r = r + block[:, i:i + 8]
            res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
            for i in range(lim, ln):
                res = res + block[:, i]
        out[sel] = res
    return out


def pairwise_sum(a):
    """numpy's float64 pairwise sum of a (1-D float64), every addition spelled out"""
    a = np.asarray(a, dtype=np.float64)
    if len(a) == 0:
        return 0.0
    leaves, tree = leaves_of(len(a))
    sums = leaf_sums(a, leaves)

    def value(t):
        if isinstance(t, tuple):
            return value(t[0]) + value(t[1])
        return sums[t]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float64(value(tree))


PIECE = 8192


def reduce64(a):
    """np.add.reduce of a contiguous float64 array: the pieces' pairwise sums added up in order"""
    total = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for off in range(0, len(a), PIECE):
            total = total + pairwise_sum(a[off:off + PIECE])
    return total


def mean64(a):
    """np.mean of a float64 window: reduce64 / count; NaN for an empty one"""
    if len(a) == 0:
        return np.float64("nan")
    with np.errstate(invalid="ignore", over="ignore"):
        return reduce64(a) / np.float64(len(a))


def magnitudes(iq):
    """util.get_magnitudes: float32 -- fp32 multiply, add and sqrtf, widened; integer types -- C int sum with its wrap-around, double sqrt"""
    iq = np.asarray(iq)
    if iq.dtype == np.float32:
        return np.sqrt(iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).astype(np.float64)
    a = iq.astype(np.int64)
    s = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    with np.errstate(invalid="ignore"):
        return np.sqrt(s.astype(np.float64))


def norm_of(dtype):
    """sqrt(max^2 + min^2) of IQArray.min_max_for_dtype"""
    dtype = np.dtype(dtype)
    lo, hi = (-1, 1) if dtype.kind == "f" else (np.iinfo(dtype).min, np.iinfo(dtype).max)
    return np.sqrt(hi ** 2.0 + lo ** 2.0)


def records(iq, msg_off, pauses, pos, pos_off, mod, sps, divisor):
    """one record per message from a pass's flat outputs (before any padding) and the capture"""
    iq = np.asarray(iq)
    n, sps, divisor = len(iq), int(sps), int(divisor)
    out = np.zeros(len(pauses), RECORD_DTYPE)
    norm = norm_of(iq.dtype)
    for m in range(len(pauses)):
        ln = int(msg_off[m + 1] - msg_off[m])
        p = [int(v) for v in pos[pos_off[m]:pos_off[m + 1]]]
        n_pad = 0
        if mod == "ASK" and divisor > 1:
            missing = (divisor - ln % divisor) % divisor
            if missing > 0 and int(pauses[m]) >= sps * missing:
                n_pad = missing
        k = (ln + n_pad) // 2
        if n_pad:                                                          # the message's positions after the padding (see padded())
            p = p[:-1] + [p[-2] + (t + 1) * sps for t in range(n_pad)]
        mid = p[k]
        window = iq[mid:mid + sps]                                         # (Python's slice: clipped at the capture's end)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[m] = (mean64(magnitudes(window) / norm), p[0], mid, n_pad, 1)
    return out


def padded(bits, msg_off, pauses, pos, pos_off, n_pad, sps):
    """the messages after the padding, message by message: lists of (bits, pause, positions)"""
    out = []
    for m in range(len(pauses)):
        b = [int(v) for v in bits[msg_off[m]:msg_off[m + 1]]]
        p = [int(v) for v in pos[pos_off[m]:pos_off[m + 1]]]
        pause, k = int(pauses[m]), int(n_pad[m])
        if k:                                                              # the last entry is replaced, k more follow, each sps further; then the new pause
            start = p[-2]
            pause -= k * sps
            p = p[:-1] + [start + (t + 1) * sps for t in range(k)] + [start + k * sps + pause]
            b = b + [0] * k
        out.append((b, pause, p))
    return out
