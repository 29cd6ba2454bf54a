"""The estimators' reductions across ranks: numpy's float32 summation tree (csrc/pairwise.hpp has the order; csrc/shard_estimators.hip
writes the records), util.minmax, and detect_center's trimmed sequence -- every result a pure function of gathered data, so every rank
that evaluates one gets the same bits.  `ShardedPipeline.detect_noise_level` / `detect_center` (pipeline.py) say what is gathered."""
import numpy as np

PW_PIECE, PW_LEAF = 8192, 128               # kPwChunk, kPwLeaf
PW_REC_HEAD, PW_REC_FIRST, PW_REC_LAST, PW_REC_TAIL, PW_REC_PIECES = 8, 136, 264, 392, 520      # URHGPU_PW_REC_* (include/urhgpu.h)
HIST_GATHER_BINS = 1 << 22                  # bins per all-gather of detect_center's histogram (32 MiB of int64 per rank)


def pairwise_inside_pieces(g_off: int, m_local: int, m_total: int):
    """[pa, pb): the full pieces of PW_PIECE elements that lie wholly inside [g_off, g_off + m_local) of a sequence of m_total"""
    pa = -(-g_off // PW_PIECE)
    pb = min((g_off + m_local) // PW_PIECE, m_total // PW_PIECE)
    return pa, max(pa, pb)


def pairwise_record_words(g_off: int, m_local: int, m_total: int) -> int:
    """length in float32 words of the record urhgpu_pairwise_partial_f32_dev writes for that range"""
    pa, pb = pairwise_inside_pieces(g_off, m_local, m_total)
    return PW_REC_PIECES + pb - pa


def pairwise_piece_leaves(p: int, m_total: int):
    """the leaves of piece p as (offset in the piece, length): 64 leaves of 128 for a full piece, pw's recursive split (the left part
    is n // 2 rounded down to a multiple of 8) for the irregular last one"""
    if p < m_total // PW_PIECE:
        return [(k * PW_LEAF, PW_LEAF) for k in range(PW_PIECE // PW_LEAF)]
    out = []

    def split(off, n):
        if n <= PW_LEAF:
            out.append((off, n))
            return
        n2 = n // 2
        n2 -= n2 % 8
        split(off, n2)
        split(off + n2, n - n2)
    split(0, m_total % PW_PIECE)
    return out


def pairwise_leaf_sum(a) -> np.float32:
    """pw over one leaf (len(a) <= PW_LEAF) in float32, as pw_leaf (csrc/pairwise.hpp): 8 strided accumulators, their fixed tree, the
    len % 8 tail in order; fewer than 8 elements: in order from 0"""
    a = np.asarray(a, dtype=np.float32)
    n = len(a)
    with np.errstate(all="ignore"):
        if n < 8:
            res = np.float32(0.0)
            for v in a:
                res = np.float32(res + v)
            return res
        nb = n - n % 8
        r = np.add.accumulate(a[:nb].reshape(-1, 8), axis=0, dtype=np.float32)[-1]       # r[j] += a[i + j], row after row
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) +
                         np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[nb:]:
            res = np.float32(res + v)
        return res


def pairwise_tree(leaf_sums, lengths) -> np.float32:
    """pw's additions above the leaves: leaf_sums[i] is the sum of a leaf of lengths[i] elements, in order"""
    vals = [np.float32(v) for v in leaf_sums]
    pos = 0

    def node(n):
        nonlocal pos
        if n <= PW_LEAF:
            v = vals[pos]
            pos += 1
            return v
        n2 = n // 2
        n2 -= n2 % 8
        left = node(n2)
        right = node(n - n2)
        return np.float32(left + right)
    with np.errstate(all="ignore"):
        return node(int(sum(lengths)))


def _record_headers(records):
    recs = np.ascontiguousarray(records, dtype=np.float32)
    recs = recs.reshape(len(recs), -1)
    hdr = np.ascontiguousarray(recs[:, 0:4]).view(np.int64)
    return recs, [int(v) for v in hdr[:, 0]], [int(v) for v in hdr[:, 1]]


def pairwise_combine(records, m_total: int) -> np.float32:
    """np.add.reduce of a float32 sequence of m_total elements from the ranks' records (urhgpu_pairwise_partial_f32_dev; rank order,
    rows padded to one length): a pure function of its arguments, so every rank that evaluates it gets the same bits.  Leaves that
    a shard boundary cuts are finished from the ranks' raw elements with pw_leaf's arithmetic, pieces that one cuts from their leaf
    sums, and the pieces are accumulated left to right -- all in float32 (numpy float32 scalars: no excess precision)."""
    recs, g_offs, m_locals = _record_headers(records)
    m_total = int(m_total)
    if m_total <= 0:
        return np.float32(0.0)
    ranks = [r for r in range(len(recs)) if m_locals[r] > 0]
    at = 0
    for r in ranks:
        if g_offs[r] != at:
            raise ValueError("pairwise_combine: the ranks' ranges do not tile the sequence")
        at += m_locals[r]
    if at != m_total:
        raise ValueError("pairwise_combine: the ranks' ranges do not tile the sequence")
    n_pieces = -(-m_total // PW_PIECE)
    sums = np.zeros(n_pieces + 1, dtype=np.float32)          # sums[0]: the 0 np.add.reduce starts from
    have = np.zeros(n_pieces, dtype=bool)
    for r in ranks:
        pa, pb = pairwise_inside_pieces(g_offs[r], m_locals[r], m_total)
        sums[1 + pa:1 + pb] = recs[r, PW_REC_PIECES:PW_REC_PIECES + pb - pa]
        have[pa:pb] = True
    ends = np.array([g_offs[r] + m_locals[r] for r in ranks], dtype=np.int64)
    for p in np.nonzero(~have)[0].tolist():
        leaves = pairwise_piece_leaves(p, m_total)
        vals = []
        for off, ln in leaves:
            l0, l1 = p * PW_PIECE + off, p * PW_PIECE + off + ln
            k = int(np.searchsorted(ends, l0, side="right"))      # the rank that holds element l0
            r = ranks[k]
            if ends[k] >= l1:                                      # the leaf lies wholly inside that rank
                area = PW_REC_FIRST if p == g_offs[r] // PW_PIECE else PW_REC_LAST
                vals.append(recs[r, area + (off + 63) // 64])
                continue
            raw = []
            while k < len(ranks) and g_offs[ranks[k]] < l1:
                r = ranks[k]
                lo, hi = max(l0, g_offs[r]), min(l1, int(ends[k]))
                src = PW_REC_HEAD if l0 < g_offs[r] else PW_REC_TAIL
                raw.append(recs[r, src:src + hi - lo])
                k += 1
            vals.append(pairwise_leaf_sum(np.concatenate(raw)))
        sums[1 + p] = pairwise_tree(vals, [ln for _, ln in leaves])
    with np.errstate(all="ignore"):
        return np.add.accumulate(sums, dtype=np.float32)[-1]      # ((0 + piece 0) + piece 1) + ...: left to right


def minmax_combine(records):
    """util.minmax (util.pyx:20-36) of the whole sequence from the records' words 4-6: seeded with the sequence's first element, a NaN
    never replaces a value -- so a NaN first element stays, and any other is ignored.  Returns (min, max) as floats, None when every
    rank is empty."""
    recs, _, m_locals = _record_headers(records)
    ranks = [r for r in range(len(recs)) if m_locals[r] > 0]
    if not ranks:
        return None
    mn = mx = recs[ranks[0], 6]
    for r in ranks:
        if recs[r, 4] < mn:
            mn = recs[r, 4]
        if recs[r, 5] > mx:
            mx = recs[r, 5]
    return float(mn), float(mx)


def center_parts(kept_counts, max_size=None):
    """detect_center's trimmed sequence S = R[int(0.05 K) : int(0.95 K)] (cut to max_size) of the ranks' kept samples R, from the gathered
    kept counts: (m, [(local begin, g_r, m_r) per rank]) -- rank r's part of S is kept_r[begin : begin + m_r], elements [g_r, g_r + m_r) of
    S (m_r may be 0).  A pure function of the gathered counts."""
    counts = [int(v) for v in kept_counts]
    total = sum(counts)
    a, b = int(0.05 * total), int(0.95 * total)                    # AutoInterpretation.py:231
    m = b - a
    if max_size is not None and m > max_size:                      # :233-234
        m = int(max_size)
    parts, c0 = [], 0
    for k in counts:
        lo, hi = max(c0, a), min(c0 + k, a + m)
        if hi > lo:
            parts.append((lo - c0, lo - a, hi - lo))
        else:
            parts.append((0, min(max(c0 - a, 0), m), 0))
        c0 += k
    return m, parts
