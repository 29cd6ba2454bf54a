"""Boundary sets for the message records of a sharded capture, shared by tests/test_shard_msg_records_host.py and
tests/test_shard_msg_records_gpu.py: equal cuts, seeded random cuts, and cuts computed from a fixture's own records (the model of
tests/model_msg_records.py on what the reference recorded) so that a boundary falls at and around a message's middle window, at its first
position, inside its closing pause and inside its padded part; ranks of 2 and 5 samples inside a window; a message spread over three ranks.
Every shard has at least 2 samples (the pass's own limit).  Also the comparison of two record arrays, field by field."""
import numpy as np

import model_msg_records as mm


def whole_records(g, divisor):
    """the records of the whole capture: the model on the reference's recorded (unpadded) outputs"""
    m, plain = g["meta"], g["want"][1]
    return mm.records(g["iq"], plain["msg_off"], plain["pauses"], plain["pos"], plain["pos_off"], m["modulation_type"], m["samples_per_symbol"], divisor)


def edges_ok(edges, n):
    return edges[0] == 0 and edges[-1] == n and all(b - a >= 2 for a, b in zip(edges, edges[1:]))


def equal_edges(n, world):
    per = -(-n // world)
    return [min(n, r * per) for r in range(world)] + [n]


def random_edges(rng, n, world):
    if n < 2 * world:
        return None
    for _ in range(50):
        e = [0] + sorted(int(c) for c in rng.integers(2, n - 1, world - 1)) + [n]
        if edges_ok(e, n):
            return e
    return None


def picked_messages(n_msg):
    return sorted({0, 1, n_msg // 2, n_msg - 1} & set(range(n_msg)))


def targeted_edges(g, divisor):
    """{name: edges} from the fixture's own records"""
    m, plain = g["meta"], g["want"][1]
    n, sps = len(g["iq"]), int(m["samples_per_symbol"])
    rec = whole_records(g, divisor)
    out = {}

    def add(name, *cuts):
        e = [0] + sorted(set(int(c) for c in cuts)) + [n]
        if edges_ok(e, n):
            out[name] = e
    for i in picked_messages(len(rec)):
        mid, first, n_pad = int(rec["mid_pos"][i]), int(rec["first_pos"][i]), int(rec["n_pad"][i])
        ent = plain["pos"][plain["pos_off"][i]:plain["pos_off"][i + 1]]
        for tag, at in (("mid", mid), ("mid+1", mid + 1), ("mid+half", mid + sps // 2), ("mid+sps-1", mid + sps - 1), ("mid+sps", mid + sps), ("first", first)):
            add(f"m{i}:{tag}", at)
        if len(ent) >= 2 and plain["pauses"][i] > 1:
            add(f"m{i}:in-pause", int(ent[-2]) + int(plain["pauses"][i]) // 2)
        if n_pad and len(ent) >= 2:
            add(f"m{i}:in-pad", int(ent[-2]) + (n_pad * sps) // 2 + 1)
            add(f"m{i}:pad-start", int(ent[-2]) + 1)
        if sps >= 9:
            add(f"m{i}:ranks-of-2-and-5", mid + 1, mid + 3, mid + 8)              # the window spans at least four shards
        if len(ent) >= 8:
            span = int(ent[-3]) - first
            add(f"m{i}:three-ranks", first + span // 3, first + 2 * span // 3)    # the middle rank holds bits of this message only: it closes nothing
            add(f"m{i}:five-ranks", *[first + k * span // 5 for k in range(1, 5)])
    return out


def boundary_sets(name, g, divisor, n_random=2, worlds=(2, 3, 4, 8)):
    """{set name: edges}: equal cuts for 2, 3 and 8 ranks, seeded random cuts, the targeted ones"""
    n = len(g["iq"])
    out = {"one-rank": [0, n]}
    for world in (2, 3, 8):
        e = equal_edges(n, world)
        if edges_ok(e, n):
            out[f"equal-{world}"] = e
    rng = np.random.default_rng(sum(name.encode()) * 131 + divisor)
    for world in worlds:
        for k in range(n_random):
            e = random_edges(rng, n, world)
            if e is not None:
                out[f"random-{world}-{k}"] = e
    out.update(targeted_edges(g, divisor))
    if name == "w9000-float32":
        mid = int(whole_records(g, divisor)["mid_pos"][0])
        e = [0] + [mid + 20 * k + 1 for k in range(1, 8)] + [n]               # one window crosses seven boundaries
        assert edges_ok(e, n) and e[-2] < min(mid + 9000, n)
        out["window-over-8-ranks"] = e
    return out


def assert_same_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k in ("first_pos", "mid_pos", "n_pad", "flag"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])
    assert np.ascontiguousarray(got["rssi"]).tobytes() == np.ascontiguousarray(want["rssi"]).tobytes(), (what, got["rssi"][:8], want["rssi"][:8])


def outside_windows(rec, counts, edges, sps):
    """from the whole capture's records and the number of records per rank: (messages whose window is not wholly inside the shard of the
    rank that closes them, those among them that are NOT the first message their rank closes)"""
    n = edges[-1]
    outside, later = [], []
    at = 0
    for r, c in enumerate(counts):
        for j in range(c):
            mid = int(rec["mid_pos"][at + j])
            lo, hi = min(mid, n), min(mid + sps, n)
            if hi > lo and not (edges[r] <= lo and hi <= edges[r + 1]):
                outside.append(at + j)
                if j > 0:
                    later.append(at + j)
        at += c
    return outside, later
