"""numpy model of the chunked float32 column sum of urh_amd/csrc/dc_correct.hip: guess, two serial paths per chunk,
translate or re-evaluate.  The same decisions as the kernels, on arrays: all chunks of both columns are speculated in lockstep (one vectorised float32
addition per sample position), the stitch walks the chunks in order.  np.cumsum of a 1-D float32 array is the sequential recurrence, which is
what a re-evaluated chunk costs here.

    mean, out, stats = dc_correct_f32(x)      stats = {"chunks", "same", "moved", "redo"}
"""
import numpy as np

CHUNK = 4096
DIRECT_MAX = 2 * CHUNK
ABS = np.uint32(0x7FFFFFFF)
EXP = np.uint32(0x7F800000)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def speculate(x, guess):
    """x: float32 (N, 2); guess: float32 (n_chunks, 2).  The records of every (chunk, column): entry, exit, mn, mx (uint32), flip (bool)."""
    n = len(x)
    n_chunks = len(guess)
    pad = np.zeros((n_chunks * CHUNK, 2), np.float32)
    pad[:n] = x
    xs = pad.reshape(n_chunks, CHUNK, 2)
    live = (np.arange(n_chunks * CHUNK).reshape(n_chunks, CHUNK) < n)
    s = guess.astype(np.float32).copy()
    entry = _bits(s).copy()
    mn = entry & ABS
    mx = mn.copy()
    flip = np.zeros(s.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(CHUNK):
            on = live[:, i][:, None]
            if not on.any():
                break
            xi = xs[:, i, :]
            r = (s + xi).astype(np.float32)
            b = _bits(r)
            a = b & ABS
            mn = np.where(on, np.minimum(mn, a), mn)
            mx = np.where(on, np.maximum(mx, a), mx)
            flip |= on & (((b ^ entry) >> np.uint32(31)) != 0)
            s = np.where(on, r, s)
    return {"entry": entry, "exit": _bits(s).copy(), "mn": mn, "mx": mx, "flip": flip}


def derive(recs, c, col, t):
    """The true exit (bits) of chunk c entered with the bits t, where its two records (the path from the guess, the path from the guess's
    neighbour) allow it; else None.  -> (bits, kind)"""
    for rec in recs:
        if t == int(rec["entry"][c, col]):
            return int(rec["exit"][c, col]), "same"
    if (t & 0x7FFFFFFF) > 0x7F800000:
        return t, "moved"                                  # a NaN sum absorbs whatever follows
    rec = recs[(t ^ int(recs[0]["entry"][c, col])) & 1]    # the path an even number of ulps away: it meets every tie as the true path does
    g, x = int(rec["entry"][c, col]), int(rec["exit"][c, col])
    if (t ^ g) >> 31 or rec["flip"][c, col]:
        return None
    ga = g & 0x7FFFFFFF
    lo = ga & 0x7F800000
    hi = lo | 0x007FFFFF
    mn, mx = int(rec["mn"][c, col]), int(rec["mx"][c, col])
    if lo == 0x7F800000 or mn < lo or mx > hi:
        return None
    d = (t & 0x7FFFFFFF) - ga
    if abs(d) + 1 > min(mn - lo, hi - mx):
        return None
    assert d % 2 == 0
    return (x & 0x80000000) | ((x & 0x7FFFFFFF) + d), "moved"


def serial(chunk_col, t):
    """the chunk evaluated from its true entry: the sequential float32 recurrence"""
    with np.errstate(all="ignore"):
        start = np.array([t], np.uint32).view(np.float32)
        return int(np.cumsum(np.concatenate([start, chunk_col]), dtype=np.float32)[-1:].view(np.uint32)[0])


def column_sums(x, guess=None):
    """the two sequential float32 sums of x (N, 2) by the chunked scheme -> (float32[2], stats)"""
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    n_chunks = (n + CHUNK - 1) // CHUNK
    stats = {"chunks": 0, "same": 0, "moved": 0, "redo": 0}
    t = [0, 0]                                              # +0.0
    if n <= DIRECT_MAX:
        for col in range(2):
            t[col] = serial(x[:, col], 0)
    else:
        stats["chunks"] = n_chunks
        if guess is None:
            with np.errstate(all="ignore"):
                sums = np.add.reduceat(x.astype(np.float64), np.arange(0, n, CHUNK), axis=0)
                prefix = np.concatenate([np.zeros((1, 2)), np.cumsum(sums, axis=0)[:-1]])
                guess = prefix.astype(np.float32)
        with np.errstate(all="ignore"):
            rec = (speculate(x, guess), speculate(x, (_bits(guess) + np.uint32(1)).view(np.float32)))
        for col in range(2):
            for c in range(n_chunks):
                got = derive(rec, c, col, t[col])
                if got is None:
                    t[col] = serial(x[c * CHUNK:(c + 1) * CHUNK, col], t[col])
                    stats["redo"] += 1
                else:
                    t[col] = got[0]
                    stats[got[1]] += 1
    return np.array(t, np.uint32).view(np.float32), stats


def dc_correct_f32(x, guess=None):
    x = np.ascontiguousarray(x, np.float32)
    s, stats = column_sums(x, guess)
    with np.errstate(all="ignore"):
        mean = (s.astype(np.float64) / float(len(x))).astype(np.float32)
        return mean, x - mean, stats


def dc_correct_int(x):
    """integers: exact sum, float64 mean, the difference truncated into an int32 and its low bits kept"""
    s = x.astype(np.int64).sum(axis=0)
    mean = s.astype(np.float64) / float(len(x))
    d = np.trunc(x.astype(np.float64) - mean).astype(np.int64)
    bits = x.dtype.itemsize * 8
    low = d & ((1 << bits) - 1)
    if x.dtype.kind == "i":
        low = np.where(low >= 1 << (bits - 1), low - (1 << bits), low)
    return mean, low.astype(x.dtype)
