"""DC correction across the shards: `ShardedPipeline.dc_correct` subtracts the mean of the WHOLE capture from every shard, bit-equal with
numpy's `x - np.mean(x, axis=0)`.  Integers: one all-gather of the ranks' exact int64 column sums.  float32: the mean is the strictly
sequential float32 sum of the capture, carried across the ranks like the Costas state (csrc/dc_correct.hip writes the records):

    A. sums        three 8-byte words per rank: n_local and the two column sums (float64 for float32 captures: the guesses)
    B. records     every rank speculates its shard from fl32(the float64 sum of the ranks before it) and from that guess's neighbour and
                   gathers, per column and path, {entry, exit, room}: the exit holds for every entry an even number of ulps, at most `room`,
                   from the path's (64 bytes per rank)
    C. compose     `dc_compose` (a pure function of the gathered bytes) walks the ranks with the true entry; where a record does not
                   reach, that rank re-stitches from its true entry and hands its exit over in one more all-gather of 8 bytes per rank
    D. finish      mean = fl32(double(sum) / double(n_total)); every rank subtracts it from its shard and from the raw samples handed
                   over with it (`also`)

Two all-gathers when every record holds, world + 1 at most; how many depends on gathered bytes only."""
import numpy as np

# a rank's records: [column][path] x {entry bits, exit bits, room, flags} as uint32 (URHGPU_DC_RECORD_BYTES = 64)
DC_IDENTITY = 1                             # flags: the shard holds no sample, its exit is its entry


def dc_compose(records, handoff=None):
    """Carry numpy's sequential float32 column sums across the shards: a pure function of the gathered shard records ((world, 2, 2, 4)
    uint32: per column and speculated path {entry bits, exit bits, room, flags}, rank order) and of the exits handed over so far
    (handoff: {rank: (bits I, bits Q)}), so every rank that evaluates it takes the same branch.  Rank 0 enters with +0.0.  A shard's
    exit follows from its records where the true entry equals a path's entry (the recorded exit), where it lies D ulps from the path an
    even number of ulps away, on the same side of zero, with |D| <= room (the recorded exit moved by D: every chunk on the path stays
    inside its binade, and paths an even distance apart round every tie alike), where the shard is empty, and where the sum is already
    NaN (it stays).  Returns (entries, pending, total): entries[r] = the true entry of shard r as (bits I, bits Q), None where not known
    yet; pending = the first rank one of whose columns the records cannot carry (its entry is known: it re-stitches both columns from
    it and hands its exits over), None when every entry is known; total = the sum's bits (I, Q) when pending is None."""
    rec = np.ascontiguousarray(np.asarray(records)).view(np.uint32).reshape(-1, 2, 2, 4)
    handoff = handoff or {}
    entries = [None] * len(rec)
    t = (0, 0)                                            # +0.0: numpy's accumulator starts there
    for r in range(len(rec)):
        entries[r] = t
        if r in handoff:
            t = (int(handoff[r][0]), int(handoff[r][1]))
            continue
        nxt = []
        for col in range(2):
            e = _dc_exit(rec[r, col], t[col])
            if e is None:
                return entries, r, None
            nxt.append(e)
        t = tuple(nxt)
    return entries, None, t


def _dc_exit(paths, t):
    """the exit of one column of a shard entered with the bits t, from its two path records; None where they do not give it"""
    if int(paths[0, 3]) & DC_IDENTITY:
        return t
    for p in paths:
        if t == int(p[0]):
            return int(p[1])
    if (t & 0x7FFFFFFF) > 0x7F800000:
        return t                                          # a NaN sum absorbs whatever follows
    p = paths[(t ^ int(paths[0, 0])) & 1]                 # the path an even number of ulps away
    entry, leave, room = int(p[0]), int(p[1]), int(p[2])
    if (t ^ entry) >> 31:
        return None
    d = (t & 0x7FFFFFFF) - (entry & 0x7FFFFFFF)
    if abs(d) > room:
        return None
    return (leave & 0x80000000) | ((leave & 0x7FFFFFFF) + d)
