"""Message records across the shards (csrc/msg_records.hip: k_shard_rec_summary writes the words, k_shard_msg_records takes the
descriptor): `ShardedPipeline.message_records`, called on every rank after `iq_to_bits` with the same shard and the pass's result, gives one
urhgpu_msg_record per message that closes on the rank (ASK padding, first and middle position, RSSI); the ranks' arrays concatenated in rank
order (`stitch_records`) are the single-GPU records bit for bit, and `message_data` turns pieces and records into the list of
protocol.MessageData.  Only the FIRST message a rank closes can reach outside its shard (every later one starts behind a pause row that ends
in the shard and is closed by a pause that ends in it), so what crosses the ranks is small:

    1. summary     ten 8-byte words per rank (REC_* below; include/urhgpu.h): pos_base, n_local, messages closed, bits / position entries
                   before the first and behind the last close, the first closed message's pause, "capacities held", position entries
                   -> `records_plan`: L, np, n_pad, the middle index of every rank's first message and who holds its entries 0 and rel
    2. look-up     2 x world position entries, every rank fills in the ones it holds -> first_pos, mid_pos and the window of every first message
    3. windows     only if a first window is not wholly inside its closing rank's shard: the raw samples of those windows, every rank the part
                   its shard holds; the closing rank assembles its window contiguously

Two all-gathers in the common case, three at most, none for one rank; which, depends on gathered words only."""
import numpy as np

REC_SUMMARY_WORDS = 10                      # URHGPU_SHARD_REC_SUMMARY_WORDS
(REC_POS_BASE, REC_N_LOCAL, REC_N_MSG, REC_HEAD_BITS, REC_HEAD_POS, REC_TAIL_BITS, REC_TAIL_POS, REC_FIRST_PAUSE, REC_HELD, REC_N_POS) = range(10)
REC_FIRST_WORDS = 8                         # URHGPU_SHARD_REC_FIRST_WORDS: {closes, L, np, n_pad, first_pos, mid_pos, ok, window assembled}


def records_plan(words, n_total, samples_per_symbol, divisor):
    """The first message of every closing rank from the gathered summary words ((world, REC_SUMMARY_WORDS) int64, rank order): a pure
    function of its arguments, so every rank that evaluates it takes the same branch.  Raises ValueError where the shards do not tile
    [0, n_total).  divisor: message_length_divisor for an ASK pass, 1 otherwise.  Returns a list with one entry per rank: None where the
    rank closes no message, else dict(L, np, pause, n_pad, k, rel, add, ok, first, mid) -- L bits and np position entries summed over the
    ranks since the previous close, the padding decision and the middle index as k_msg_records takes them (rel = np - 2 and
    add = (k - rel) * sps where the middle lies in the padded part, rel = k and add = 0 otherwise), first / mid = (rank, local index) of the
    position entries 0 and rel; ok False (first / mid None) where a contributing rank exceeded a capacity or the entries do not exist."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(-1, REC_SUMMARY_WORDS)
    sps, divisor = int(samples_per_symbol), int(divisor)
    at = 0
    for row in w:
        if int(row[REC_POS_BASE]) != at or int(row[REC_N_LOCAL]) < 0:
            raise ValueError("message_records: the ranks' shards do not tile the capture")
        at += int(row[REC_N_LOCAL])
    if at != int(n_total):
        raise ValueError(f"message_records: the ranks hold {at} samples, the capture has {int(n_total)}")
    plan, prev = [None] * len(w), -1
    for r, row in enumerate(w):
        if int(row[REC_N_MSG]) <= 0:
            continue
        # the ranks that contribute, in order: (rank, local index of its first entry, entries, bits)
        parts = []
        if prev >= 0:
            parts.append((prev, int(w[prev, REC_N_POS] - w[prev, REC_TAIL_POS]), int(w[prev, REC_TAIL_POS]), int(w[prev, REC_TAIL_BITS])))
        parts += [(q, 0, int(w[q, REC_HEAD_POS]), int(w[q, REC_HEAD_BITS])) for q in range(prev + 1, r + 1)]
        held = all(int(w[q, REC_HELD]) == 1 for q, _, _, _ in parts)
        L, n_pos, pause = sum(b for _, _, _, b in parts), sum(c for _, _, c, _ in parts), int(row[REC_FIRST_PAUSE])
        n_pad = 0
        if divisor > 1 and L >= 0:
            missing = (divisor - L % divisor) % divisor
            if missing > 0 and pause >= sps * missing:
                n_pad = missing
        k = (L + n_pad) // 2
        in_pad = n_pad > 0 and k > n_pos - 2
        rel = n_pos - 2 if in_pad else k
        ok = held and L >= 0 and n_pos >= 1 and 0 <= rel < n_pos and all(c >= 0 and a >= 0 for _, a, c, _ in parts)

        def locate(e):
            for q, a, c, _ in parts:
                if e < c:
                    return q, a + e
                e -= c
        plan[r] = dict(L=L, np=n_pos, pause=pause, n_pad=n_pad, k=k, rel=rel, add=(k - rel) * sps if in_pad else 0, ok=ok,
                       first=locate(0) if ok else None, mid=locate(rel) if ok else None)
        prev = r
    return plan


def records_requests(plan, rank):
    """the look-up a rank answers: int64 (2 * world,), slot 2r / 2r + 1 = the LOCAL index of entry 0 / rel of rank r's first message where
    `rank` holds it, -1 elsewhere"""
    idx = np.full(2 * len(plan), -1, np.int64)
    for r, m in enumerate(plan):
        if m is not None and m["ok"]:
            for slot, (q, at) in ((2 * r, m["first"]), (2 * r + 1, m["mid"])):
                if q == rank:
                    idx[slot] = at
    return idx


def _py_slice(start, stop, n):
    """Python's a[start:stop] on n elements: (where the slice begins, how many elements it has)"""
    a = max(start + n, 0) if start < 0 else min(start, n)
    b = max(stop + n, 0) if stop < 0 else min(stop, n)
    return a, max(b - a, 0)


def records_windows(plan, words, values, n_total, samples_per_symbol):
    """first_pos, mid_pos and the window of every first message from the plan and the gathered look-up ((world, 2 * world) int64): a pure
    function of gathered data.  Returns (firsts, outside): firsts[r] = None or dict(first_pos, mid_pos, lo, w, slot) -- the window is
    samples [lo, lo + w) of the capture, clipped at the CAPTURE's end, slot = its index among the exchanged windows or -1 where it lies
    wholly inside rank r's shard (or is empty); outside = the closing ranks whose window is exchanged, in order."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(-1, REC_SUMMARY_WORDS)
    v = np.ascontiguousarray(np.asarray(values)).view(np.int64).reshape(len(w), 2 * len(w))
    firsts, outside = [None] * len(w), []
    for r, m in enumerate(plan):
        if m is None or not m["ok"]:
            continue
        first_pos = int(v[m["first"][0], 2 * r])
        mid_pos = int(v[m["mid"][0], 2 * r + 1]) + m["add"]
        lo, cnt = _py_slice(mid_pos, mid_pos + int(samples_per_symbol), int(n_total))
        a, b = int(w[r, REC_POS_BASE]), int(w[r, REC_POS_BASE] + w[r, REC_N_LOCAL])
        slot = -1
        if cnt > 0 and not (a <= lo and lo + cnt <= b):
            slot = len(outside)
            outside.append(r)
        firsts[r] = dict(first_pos=first_pos, mid_pos=mid_pos, lo=lo, w=cnt, slot=slot)
    return firsts, outside


def stitch_records(records):
    """the ranks' record arrays (rank order) as the one array of the whole capture's messages"""
    from ..protocol import RECORD_DTYPE
    parts = [np.asarray(r, dtype=RECORD_DTYPE) for r in records]
    return np.concatenate(parts) if parts else np.zeros(0, RECORD_DTYPE)


def message_data(pieces, records, p, sample_rate=1e6, timestamp=0.0):
    """The list of protocol.MessageData of a sharded pass -- what BitsResult.message_data() gives for the single-GPU one -- from the ranks'
    pieces (as `stitch` takes them) and their records (the ranks' arrays in rank order, or one stitched array).  Raises as the single-GPU
    route does (UrhGpuError, ERR_CAPACITY) where a record says that a capacity was exceeded (flag 0), and RuntimeError naming the flag for
    -2 (a window left its rank's shard) and -1."""
    from .. import _lib
    from ..protocol import messages_from_records
    from .pipeline import stitch
    rec = stitch_records(records) if isinstance(records, (list, tuple)) else np.asarray(records)
    flat = stitch(pieces)[1:]
    if len(rec) != len(flat[2]):
        raise ValueError(f"message_data: {len(rec)} records for {len(flat[2])} messages")
    if not (rec["flag"] == 1).all():
        bad = np.nonzero(rec["flag"] != 1)[0]
        flag = int(rec["flag"][bad[0]])
        where = f"{len(bad)} of {len(rec)} records are not valid (first: message {int(bad[0])}, flag {flag}, record {rec[bad[0]]})"
        if flag == 0:
            raise _lib.UrhGpuError(_lib.ERR_CAPACITY, f"output capacity too small on a rank that contributes to the message: {where}")
        if flag == -2:
            raise RuntimeError(f"message_records: the middle window of a message that is not the first one its rank closes left the rank's shard "
                               f"(flag -2; nothing outside the shard was read, no RSSI): {where}")
        raise RuntimeError(f"message_records: the summation of a window gave up (flag -1): {where}")
    return messages_from_records(flat, rec, p, sample_rate, timestamp)
