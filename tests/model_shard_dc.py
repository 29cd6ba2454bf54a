"""Executable model (numpy, CPU tensors) of the engine methods behind ShardedPipeline.dc_correct (urh_amd/shard_engine.py: dc_own, dc_whole,
dc_sums, dc_spec, dc_resolve, dc_apply, dc_stats) and of the shard records of urh_amd/csrc/dc_correct.hip, built on the chunk model of
tests/model_dc.py: the CPU suite drives the orchestration and dc_compose of urh_amd/sharding.py with it.

A shard record is, per column and speculated path, {entry bits, exit bits, room, flags}: the shard stitched from `entry` leaves with `exit`,
and so it does, moved by D, from every entry an even D ulps away with |D| <= room -- every chunk on the path is then still derived by
the record that derived it.  A chunk entered d ulps from its chosen record's entry, whose path keeps m = min(mn - lo, hi - mx) ulps from
its binade's edges, allows m - 1 - |d|; a chunk that was re-evaluated, taken by exact hit from a record that cannot be translated, or
entered with a NaN sum allows nothing."""
import numpy as np
import torch

import model_dc as D

ROOM_MAX = 0x7FFFFFFE
IDENTITY = 1


def _np(t):
    return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _rows(t):
    """(n, 2) view of a shard in a sample type or complex64 (n,)"""
    a = _np(t)
    return a.view(np.float32).reshape(-1, 2) if a.dtype == np.complex64 else a


def margin(rec, c, col, t):
    """m of the record's path for an entry on t's side of zero, -1 where the record cannot be translated"""
    g = int(rec["entry"][c, col])
    if (t ^ g) >> 31 or rec["flip"][c, col]:
        return -1
    lo = g & 0x7F800000
    hi = lo | 0x007FFFFF
    mn, mx = int(rec["mn"][c, col]), int(rec["mx"][c, col])
    if lo == 0x7F800000 or mn < lo or mx > hi:
        return -1
    return min(mn - lo, hi - mx)


def derive_room(recs, c, col, t):
    """dc_derive_room (dc_correct.hip): (exit bits, kind, room of this chunk), None where the chunk has to be re-evaluated"""
    for rec in recs:
        if t == int(rec["entry"][c, col]):
            return int(rec["exit"][c, col]), "same", max(margin(rec, c, col, t) - 1, 0)
    if (t & 0x7FFFFFFF) > 0x7F800000:
        return t, "moved", 0
    rec = recs[(t ^ int(recs[0]["entry"][c, col])) & 1]
    m = margin(rec, c, col, t)
    d = (t & 0x7FFFFFFF) - (int(rec["entry"][c, col]) & 0x7FFFFFFF)
    if m < 0 or abs(d) + 1 > m:
        return None
    x = int(rec["exit"][c, col])
    return (x & 0x80000000) | ((x & 0x7FFFFFFF) + d), "moved", m - 1 - abs(d)


def chunk_records(x, base):
    """the two speculated paths of every chunk of the shard x (float32 (n, 2)), guessed from fl32(base + the float64 prefix of the chunk sums)"""
    n = len(x)
    with np.errstate(all="ignore"):
        sums = np.add.reduceat(x.astype(np.float64), np.arange(0, n, D.CHUNK), axis=0)
        prefix = np.concatenate([np.zeros((1, 2)), np.cumsum(sums, axis=0)[:-1]]) + np.asarray(base, np.float64)
        guess = prefix.astype(np.float32)
        return D.speculate(x, guess), D.speculate(x, (D._bits(guess) + np.uint32(1)).view(np.float32))


def stitch(x, recs, col, entry, stats):
    """the column stitched from the bits `entry` -> (exit bits, room)"""
    t, room = int(entry), ROOM_MAX
    for c in range(-(-len(x) // D.CHUNK)):
        got = derive_room(recs, c, col, t)
        if got is None:
            t, room = D.serial(x[c * D.CHUNK:(c + 1) * D.CHUNK, col], t), 0
            stats["reevaluated"] += 1
        else:
            t, room = got[0], min(room, got[2])
            stats["derived"] += 1
    return t, room & ~1


class ModelDcEngine:
    """the DC methods of an engine, on numpy arrays / CPU tensors"""

    def __init__(self):
        self._stats = {"chunks": 0, "derived": 0, "reevaluated": 0}
        self.rooms = None                                   # the last dc_spec's rooms, [column][path]

    def dc_own(self, iq_local, also, out):
        x = _rows(iq_local)
        if x.dtype not in (np.int8, np.uint8, np.int16, np.uint16, np.float32):
            raise ValueError("Unsupported dtype")
        if x.ndim != 2 or x.shape[1] != 2 or not x.flags.c_contiguous:
            raise ValueError("dc_correct: the shard must be a contiguous (n, 2) tensor")
        if out is not None and out is not iq_local:
            raise ValueError("dc_correct: out is None or the shard itself")
        for t in also:
            a = _rows(t)
            if a.dtype != x.dtype or a.ndim != 2 or a.shape[1] != 2 or not a.flags.c_contiguous:
                raise ValueError("dc_correct: `also` holds contiguous (m, 2) tensors of the shard's sample type")
        return x.dtype == np.float32

    def dc_whole(self, iq_local, out):
        x = _rows(iq_local)
        if x.dtype == np.float32:
            mean, _, st = D.dc_correct_f32(x)
            self._stats = {"chunks": st["chunks"], "derived": st["same"] + st["moved"], "reevaluated": st["redo"]}
        else:
            mean, _ = D.dc_correct_int(x)
        return self.dc_apply(iq_local, mean, out), mean

    def dc_sums(self, iq_local):
        x = _rows(iq_local)
        w = np.zeros(3, np.int64)
        w[0] = len(x)
        if x.dtype == np.float32:
            with np.errstate(all="ignore"):
                w[1:] = x.astype(np.float64).sum(axis=0).view(np.int64)
        else:
            w[1:] = x.astype(np.int64).sum(axis=0)
        return torch.from_numpy(w)

    def dc_spec(self, iq_local, base):
        x = np.ascontiguousarray(_rows(iq_local), np.float32)
        out = np.zeros((2, 2, 4), np.uint32)
        self._stats = {"chunks": -(-len(x) // D.CHUNK), "derived": 0, "reevaluated": 0}
        self._recs = chunk_records(x, base) if len(x) else None
        with np.errstate(all="ignore"):
            first = D._bits(np.asarray(base, np.float64).astype(np.float32))
        for col in range(2):
            for path in range(2):
                entry = int(first[col]) + path
                leave, room = stitch(x, self._recs, col, entry, self._stats) if len(x) else (entry, ROOM_MAX)
                out[col, path] = (entry, leave, room, 0 if len(x) else IDENTITY)
        self.rooms = out[:, :, 2].copy()
        return torch.from_numpy(out.view(np.int32))

    def dc_resolve(self, iq_local, entry):
        out = np.zeros(2, np.uint32)
        if entry is not None:
            x = np.ascontiguousarray(_rows(iq_local), np.float32)
            for col in range(2):
                out[col] = stitch(x, self._recs, col, entry[col], self._stats)[0] if len(x) else entry[col]
        return torch.from_numpy(out.view(np.int32))

    def dc_apply(self, x, mean, out):
        a = _rows(x)
        with np.errstate(all="ignore"):
            if a.dtype == np.float32:
                res = a - np.asarray(mean, np.float32)
            else:
                d = np.trunc(a.astype(np.float64) - np.asarray(mean, np.float64)).astype(np.int64)
                bits = a.dtype.itemsize * 8
                low = d & ((1 << bits) - 1)
                if a.dtype.kind == "i":
                    low = np.where(low >= 1 << (bits - 1), low - (1 << bits), low)
                res = low.astype(a.dtype)
        if out is not None:
            a[...] = res
            return x
        return res.view(np.complex64).reshape(-1) if _np(x).dtype == np.complex64 else res

    def dc_stats(self):
        return dict(self._stats)
