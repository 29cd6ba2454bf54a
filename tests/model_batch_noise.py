"""numpy model of k_batch_noise (urh_amd/csrc/batch_auto.hip): detect_noise_level of one capture of a batch, statement for statement.
  magnitudes   MagLoad<DT>::mag (magnitude.hpp): float32 -> (double)sqrtf(I * I + Q * Q) in fp32; integers -> products and sum in a wrapping C
               int, the square root in double (a negative sum: NaN)
  geometry     model_noise.chunk_geometry; chunk j = [n - (j + 1) chunk, n - j chunk) of THAT capture
  chunk sums   the kernel's order: pieces of 8192 terms, total = ((0 + pw(piece 0)) + pw(piece 1)) + ...; a piece's tree walked depth first
               (plan()), a leaf's eight strided accumulators combined by an xor butterfly over distances 1, 2, 4, the n % 8 tail in order,
               leaves below 8 terms in order; the additions run on a value stack
  decision     model_noise.decide (the body k_noise_decide and k_batch_noise share)
The arrays' first axis runs over the chunks of a capture: all of them have the same length and take the same additions.
test_batch_auto_host.py holds chunk_sums against np.add.reduce bit for bit and detect() against the oracle and the real reference."""
import numpy as np

import model_noise

PW_CHUNK, PW_LEAF = 8192, 128
MAX_LEAVES, MAX_FRAMES, MAX_VALS = 128, 16, 16


def magnitudes(iq):
    iq = np.asarray(iq)
    if iq.dtype == np.float32:
        with np.errstate(all="ignore"):
            s = (iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).astype(np.float32)      # two fp32 products, one fp32 sum: nothing contracted
            return np.sqrt(s).astype(np.float64)
    re, im = iq[:, 0].astype(np.int64), iq[:, 1].astype(np.int64)
    s = ((re * re + im * im) & 0xffffffff).astype(np.uint32).view(np.int32)          # the wrapping C int
    with np.errstate(invalid="ignore"):
        return np.sqrt(s.astype(np.float64))


def pw_split(n):
    n2 = n // 2
    return n2 - n2 % 8


def plan(length):
    """bn_plan: (leaves [(offset, length)], ops [0 = push the next leaf's sum, 1 = add the two on top]) of pw's tree over `length` terms"""
    off, ln, stage = [0], [length], [0]
    leaves, ops = [], []
    while off:
        o, l, st = off[-1], ln[-1], stage[-1]
        if l <= PW_LEAF:
            leaves.append((o, l)); ops.append(0)
            off.pop(); ln.pop(); stage.pop()
        elif st == 2:
            ops.append(1)
            off.pop(); ln.pop(); stage.pop()
        else:
            assert len(off) < MAX_FRAMES
            n2 = pw_split(l)
            stage[-1] = st + 1
            off.append(o if st == 0 else o + n2); ln.append(n2 if st == 0 else l - n2); stage.append(0)
    assert len(leaves) <= MAX_LEAVES and len(ops) <= 2 * MAX_LEAVES
    return leaves, ops


def leaf_sums(m, off, ln):
    """one leaf of every row of m (float64 (rows, terms)): eight lanes, lane j adds the terms j, j + 8, ... in order"""
    if ln < 8:
        res = np.zeros(m.shape[0])
        for i in range(ln):
            res = res + m[:, off + i]
        return res
    m8 = ln - ln % 8
    r = [m[:, off + j] for j in range(8)]
    for j in range(8):
        for i in range(8 + j, m8, 8):
            r[j] = r[j] + m[:, off + i]
    for d in (1, 2, 4):                                   # every lane adds its partner's value: lane 0 ends with ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7))
        r = [r[j] + r[j ^ d] for j in range(8)]
    res = r[0]
    for i in range(m8, ln):
        res = res + m[:, off + i]
    return res


def chunk_sums(m):
    """the kernel's sum of every row of m (float64 (rows, chunk)), one addition at a time"""
    m = np.asarray(m, dtype=np.float64)
    chunk = m.shape[1]
    total = np.zeros(m.shape[0])
    with np.errstate(all="ignore"):
        for base in range(0, chunk, PW_CHUNK):
            length = min(PW_CHUNK, chunk - base)
            leaves, ops = plan(length)
            sums = [leaf_sums(m, base + o, l) for o, l in leaves]
            stack, leaf = [], 0
            for op in ops:
                if op == 0:
                    stack.append(sums[leaf]); leaf += 1
                else:
                    y = stack.pop(); x = stack.pop()
                    stack.append(x + y)
                assert len(stack) <= MAX_VALS
            total = total + stack[0]
    return total


def chunk_stats(mags):
    """(sums, maxs, chunk), chunk 0 = the capture's last one"""
    n = len(mags)
    chunk, k = model_noise.chunk_geometry(n)
    if k == 0:
        return np.zeros(0), np.zeros(0), chunk
    rows = np.ascontiguousarray(mags[n - k * chunk:].reshape(k, chunk)[::-1])
    with np.errstate(invalid="ignore"):
        return chunk_sums(rows), np.max(rows, axis=1), chunk            # (np.max: a NaN wins)


def detect(iq):
    """(noise, flag) of a capture, as the kernel's result block has them"""
    sums, maxs, chunk = chunk_stats(magnitudes(iq))
    noise, flag, _, _, _ = model_noise.decide(sums, maxs, chunk, model_noise.max_magnitude(np.asarray(iq).dtype))
    return noise, flag
