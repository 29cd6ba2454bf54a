"""ShardedPipeline.message_records on the CPU: the orchestration and the pure functions of urh_amd/sharding.py (records_plan,
records_requests, records_windows, stitch_records, message_data) driven over ThreadComm by the executable models -- the pass is
tests/model_shard.py on the oracle's afp_demod of the fixture, the records come from tests/model_shard_msg_records.py -- against what the
REAL reference recorded (tests/golden/msg_records/) and against the model of the single-GPU records on the whole capture; the protocol
(how many all-gathers, shards that do not tile, what a rank without a message does) and the C boundary of the new entry points."""
import numpy as np
import pytest

import model_shard_estimators as M
import model_shard_msg_records as MR
import msg_record_cases as mc
import shard_record_cases as sc
from urh_amd import sharding as S


@pytest.fixture(scope="module")
def gold():
    return mc.load()


@pytest.fixture(scope="module")
def demod(oracle, gold):
    cache = {}

    def get(case):
        if case not in cache:
            g = gold[case]
            m = g["meta"]
            cache[case] = oracle.afp_demod(g["iq"], m["noise_threshold"], m["modulation_type"], 2 ** m["bits_per_symbol"], m["costas_loop_bandwidth"])
        return cache[case]
    return get


def run(g, qad, edges, divisors, held=None, pos_bases=None):
    """the pass and, for every divisor, the records, on len(edges) - 1 ranks -> per rank (piece, {divisor: records}, {divisor: last_records}, engine)"""
    m = g["meta"]
    p, n, world = mc.params(m), len(g["iq"]), len(edges) - 1
    engines = [MR.pass_and_records_engine(held=True if held is None else held[r], tile=32, span=8, chunk_tiles=2) for r in range(world)]

    def work(r, comm):
        a, b = edges[r], edges[r + 1]
        sp = S.ShardedPipeline(engines[r], comm)
        piece = sp.iq_to_bits(qad[a:b], p, pos_base=a, n_total=n)
        recs, last = {}, {}
        for d in divisors:
            try:                            # (caught here: a rank that raised out of `work` would break the barrier the others are still leaving)
                recs[d] = sp.message_records(g["iq"][a:b], piece, p, d, pos_base=a if pos_bases is None else pos_bases[r], n_total=n)
            except ValueError as exc:
                recs[d] = exc
            last[d] = sp.last_records
        return piece, recs, last, engines[r]
    return M.run_ranks(world, work)


def check(case, g, qad, name, edges):
    m = g["meta"]
    sps, world = int(m["samples_per_symbol"]), len(edges) - 1
    divisors = [int(d) for d in m["divisors"]]
    got, err = run(g, qad, edges, divisors)
    assert not any(err), (case, name, edges, err)
    pieces = [x[0] for x in got]
    seen = 0
    for d in divisors:
        what = (case, d, name, edges)
        ranks = [x[1][d] for x in got]
        assert all(r.dtype == S.stitch_records([]).dtype for r in ranks)
        rec = S.stitch_records(ranks)
        want = sc.whole_records(g, d)
        sc.assert_same_records(rec, want, what)                                    # the single-GPU records' model on the whole capture
        assert (rec["flag"] == 1).all()
        msgs = S.message_data(pieces, ranks, mc.params(m), m["sample_rate"], m["timestamp"])
        mc.assert_messages(msgs, g["want"][d], what)                               # what the REAL reference recorded
        assert [len(r) for r in ranks] == [len(pc["pauses"]) for pc in pieces]
        # the protocol: only first messages reach outside their rank's shard, and the number of all-gathers follows from that alone
        outside, later = sc.outside_windows(want, [len(r) for r in ranks], edges, sps)
        assert not later, (what, later)
        lasts = [x[2][d] for x in got]
        assert all(l == lasts[0] for l in lasts), (what, lasts)
        assert lasts[0]["windows"] == len(outside), (what, lasts[0], outside)
        assert lasts[0]["all_gathers"] == (0 if world == 1 else 3 if outside else 2), (what, lasts[0])
        seen += len(outside)
    return seen


@pytest.mark.parametrize("case", mc.names())
def test_fixtures_at_every_boundary_set(gold, demod, case):
    g = gold[case]
    big = len(g["iq"]) > 4000
    sets = sc.boundary_sets(case, g, 1, n_random=1 if big else 2)
    for d in g["meta"]["divisors"]:
        if int(d) > 1:                                                           # (the padded part exists for these only)
            sets.update({f"d{d}:{k}": v for k, v in sc.targeted_edges(g, int(d)).items() if "pad" in k})
    if len(g["iq"]) >= 16:                                                       # (every fixture: 100 samples and more)
        assert {"one-rank", "equal-2", "equal-3", "equal-8"} <= set(sets) and all(any(k.startswith(f"random-{w}-") for k in sets) for w in (2, 3, 4, 8))
    if len(g["want"][1]["pauses"]) > 0:
        assert any(k.endswith(":mid") for k in sets) and any(k.endswith(":mid+sps") for k in sets) and any(k.endswith(":first") for k in sets)
    for name, edges in sets.items():
        check(case, g, demod(case), name, edges)


def test_the_boundary_sets_hold_the_cases(gold, demod):
    """the grounds the sets were built for are really in them: windows that span three and more shards, a window over seven boundaries, a
    rank inside a message that closes nothing, boundaries inside a padded part, exchanged windows at all"""
    g = gold["w9000-float32"]
    edges = sc.boundary_sets("w9000-float32", g, 1)["window-over-8-ranks"]
    mid = int(sc.whole_records(g, 1)["mid_pos"][0])
    assert len(edges) == 9 and sum(mid < e < min(mid + 9000, len(g["iq"])) for e in edges) == 7
    assert check("w9000-float32", g, demod("w9000-float32"), "window-over-8-ranks", edges) == 1
    g = gold["pad"]
    sets = sc.targeted_edges(g, 8)
    assert any("in-pad" in k for k in sets) and any("ranks-of-2-and-5" in k for k in sets) and any("three-ranks" in k for k in sets)
    assert sum(check("pad", g, demod("pad"), k, e) for k, e in sets.items()) > 10
    name = next(k for k in sets if "three-ranks" in k)
    got, err = run(g, demod("pad"), sets[name], [8])
    assert not any(err) and len(got[1][1][8]) == 0 and len(got[1][0]["bits"]) > 0, name      # bits on the middle rank, no message closed there
    spans = [e for x in got for e in x[3].exchanged]
    rec = sc.whole_records(g, 8)
    assert all(lo in rec["mid_pos"] for lo, _ in spans)


@pytest.mark.parametrize("case", ["pad", "pad-i16", "trail", "m70", "sa5", "sf3", "fsk4", "w129-int16", "clip", "at0", "u16nan"])
def test_seeded_sweep_of_random_cuts(gold, demod, case):
    """no record carries flag -2 and only first messages are exchanged, whatever the cut: check() asserts flag == 1 on every record and
    that no window of a later message leaves its rank's shard.  The sweep runs 11 of the 37 fixtures (one of every family: padding, trailing
    message, many messages, FSK, 4-FSK, the integer types, a clipped window, a message at sample 0, NaN magnitudes), 12 seeded cuts each
    over 2, 3, 4 and 8 ranks in turn, 4 cuts for the fixtures of 4000 samples and more; every fixture is run at its equal, random and
    targeted cuts by test_fixtures_at_every_boundary_set.  With these seeds every one of the 11 exchanges at least 5 windows (summed over
    its divisors), which the last line holds: a sweep that never cut a first window would show nothing."""
    g = gold[case]
    rng = np.random.default_rng(len(case) * 977 + len(g["iq"]))
    exchanged = 0
    for it in range(12 if len(g["iq"]) < 4000 else 4):
        edges = sc.random_edges(rng, len(g["iq"]), [2, 3, 4, 8][it % 4])
        exchanged += check(case, g, demod(case), f"sweep-{it}", edges)
    assert exchanged >= 5, (case, exchanged)


def test_a_rank_that_exceeded_a_capacity_gives_flag_0(gold, demod):
    g = gold["pad"]
    edges = [0, 300, 560, len(g["iq"])]
    got, err = run(g, demod("pad"), edges, [8], held=[True, False, True])
    assert not any(err), err
    ranks = [x[1][8] for x in got]
    assert (ranks[0]["flag"] == 1).all() and len(ranks[1]) > 0 and (ranks[1]["flag"] == 0).all()
    assert ranks[2]["flag"][0] == 0 and (ranks[2]["flag"][1:] == 1).all()          # its first message began on the rank that failed
    from urh_amd import _lib
    with pytest.raises(_lib.UrhGpuError):
        S.message_data([x[0] for x in got], ranks, mc.params(g["meta"]))


def test_shards_that_do_not_tile_raise_on_every_rank(gold, demod):
    g = gold["pad"]
    edges = [0, 300, 560, len(g["iq"])]
    for bases in ([0, 301, 560], [0, 300, 300], [1, 300, 560]):
        got, err = run(g, demod("pad"), edges, [1, 8], pos_bases=bases)            # (twice: no rank is left in a collective after the first)
        assert not any(err), err
        assert all(isinstance(x[1][d], ValueError) and "message_records" in str(x[1][d]) for x in got for d in (1, 8)), (bases, got)


def test_records_plan_on_hand_written_words():
    # three ranks of 100 samples, sps 10; rank 0 closes 2 messages and keeps 3 bits / 3 entries behind the last close; rank 1 closes nothing
    # (4 bits); rank 2 closes one message after 5 more bits and 7 entries (5 bits + the two of the close), pause 35
    words = np.array([[0, 100, 2, 6, 8, 3, 3, 40, 1, 19],
                      [100, 100, 0, 4, 4, 0, 0, 0, 1, 4],
                      [200, 100, 1, 5, 7, 0, 0, 35, 1, 7]], np.int64)
    plan = S.records_plan(words, 300, 10, 1)
    assert plan[1] is None
    assert {k: plan[0][k] for k in ("L", "np", "n_pad", "k", "rel", "add", "ok", "first", "mid")} == \
        dict(L=6, np=8, n_pad=0, k=3, rel=3, add=0, ok=True, first=(0, 0), mid=(0, 3))
    assert {k: plan[2][k] for k in ("L", "np", "pause", "n_pad", "k", "rel", "first", "mid")} == \
        dict(L=12, np=14, pause=35, n_pad=0, k=6, rel=6, first=(0, 16), mid=(1, 3))
    # padded to 16: 4 bits missing, the pause holds only 3 symbols -> no padding; to 15: 3 missing -> padded, k = 7 on rank 2 at 0
    assert S.records_plan(words, 300, 10, 16)[2]["n_pad"] == 0
    p15 = S.records_plan(words, 300, 10, 15)[2]
    assert (p15["n_pad"], p15["k"], p15["rel"], p15["add"], p15["mid"]) == (3, 7, 7, 0, (2, 0))
    # a message of 1 bit padded to 8: the middle (index 4) lies in the padded part -> entry np - 2 plus 3 symbols
    one = np.array([[0, 300, 1, 1, 3, 0, 0, 200, 1, 3]], np.int64)
    p8 = S.records_plan(one, 300, 10, 8)[0]
    assert (p8["n_pad"], p8["k"], p8["rel"], p8["add"], p8["first"], p8["mid"]) == (7, 4, 1, 30, (0, 0), (0, 1))
    assert S.records_requests([p8], 0).tolist() == [0, 1]
    assert S.records_requests(plan, 1).tolist() == [-1, -1, -1, -1, -1, 3] and S.records_requests(plan, 0).tolist() == [0, 3, -1, -1, 16, -1]
    # a rank that exceeded a capacity spoils the messages it contributes to, and no others
    words[1, 8] = 0
    plan = S.records_plan(words, 300, 10, 1)
    assert plan[0]["ok"] and not plan[2]["ok"] and plan[2]["first"] is None
    # the windows: values as the ranks would have gathered them
    words[1, 8] = 1
    plan = S.records_plan(words, 300, 10, 1)
    values = np.zeros((3, 6), np.int64)
    values[0, 0], values[0, 1], values[0, 4], values[1, 5] = 5, 35, 80, 195
    firsts, outside = S.records_windows(plan, words, values, 300, 10)
    assert firsts[0] == dict(first_pos=5, mid_pos=35, lo=35, w=10, slot=-1) and firsts[1] is None
    assert firsts[2] == dict(first_pos=80, mid_pos=195, lo=195, w=10, slot=0) and outside == [2]     # [195, 205) crosses into rank 2's shard from rank 1
    values[1, 5] = 295
    firsts, outside = S.records_windows(plan, words, values, 298 + 2, 10)
    assert (firsts[2]["lo"], firsts[2]["w"], firsts[2]["slot"]) == (295, 5, -1) and outside == []     # clipped at the capture's end
    for bad, total in ((np.array([[0, 100, 0, 0, 0, 0, 0, 0, 1, 0], [101, 100, 0, 0, 0, 0, 0, 0, 1, 0]]), 201), (words, 299)):
        with pytest.raises(ValueError, match="message_records"):
            S.records_plan(bad, total, 10, 1)


def test_the_option_of_the_pass_still_raises(gold):
    sp = S.ShardedPipeline(None, S.ThreadComm(S.ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="sharded") as e:
        sp.iq_to_bits(None, mc.params(gold["pad"]["meta"]), msg_records=True)
    assert "message_records" in str(e.value)


def test_an_engine_without_the_methods_is_refused(gold):
    import model_shard
    sp = S.ShardedPipeline(model_shard.ModelShardEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0))
    with pytest.raises(NotImplementedError, match="records_summary"):
        sp.message_records(np.zeros((10, 2), np.float32), {}, mc.params(gold["pad"]["meta"]))


def test_the_c_boundary_of_the_sharded_records():
    """the ctypes prototypes exist and the calls reject null arguments before any device work"""
    import ctypes as C
    from urh_amd import _lib
    lib = _lib.load()
    for name in ("urhgpu_shard_records_summary_dev", "urhgpu_shard_records_lookup_dev", "urhgpu_shard_msg_records_dev"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    null = C.c_void_p(None)
    assert lib.urhgpu_shard_records_summary_dev(null, 10, 0, None, null) == _lib.ERR_ARG
    assert lib.urhgpu_shard_records_lookup_dev(null, None, null, 2, null) == _lib.ERR_ARG
    assert lib.urhgpu_shard_msg_records_dev(null, null, 10, 0, 10, None, None, 1, None, null, 0, null, 0, null) == _lib.ERR_ARG
    assert S.REC_SUMMARY_WORDS == MR.SUMMARY_WORDS == 10 and S.REC_FIRST_WORDS == MR.FIRST_WORDS == 8
    header = open(_lib.__file__.replace("urh_amd/_lib.py", "include/urhgpu.h")).read()
    assert "#define URHGPU_SHARD_REC_SUMMARY_WORDS 10" in header and "#define URHGPU_SHARD_REC_FIRST_WORDS 8" in header


def _gloo_worker(rank, world, port, iq, qad, meta, edges, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p, n = mc.params(meta), len(iq)
        a, b = edges[rank], edges[rank + 1]
        sp = S.ShardedPipeline(MR.pass_and_records_engine(tile=32, span=8, chunk_tiles=2), S.TorchDistComm())
        piece = sp.iq_to_bits(qad[a:b], p, pos_base=a, n_total=n)
        rec = sp.message_records(iq[a:b], piece, p, 8, pos_base=a, n_total=n)
        q.put((rank, piece, rec, sp.last_records))
    finally:
        dist.destroy_process_group()


def test_records_over_gloo(gold, demod):
    """world_size 2, one process per rank, torch.distributed gloo: a boundary inside a first message's window, three all-gathers"""
    import os
    import torch.multiprocessing as mp
    g = gold["pad"]
    edges = sc.targeted_edges(g, 8)["m3:mid+half"]
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, g["iq"], demod("pad"), g["meta"], edges, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    items = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    sc.assert_same_records(S.stitch_records([t[2] for t in items]), sc.whole_records(g, 8), "gloo")
    m = g["meta"]
    mc.assert_messages(S.message_data([t[1] for t in items], [t[2] for t in items], mc.params(m), m["sample_rate"], m["timestamp"]), g["want"][8], "gloo")
    assert [t[3] for t in items] == [{"all_gathers": 3, "windows": 1}] * 2


def test_message_data_names_the_flag(gold, demod):
    """flag 0 is a capacity (as on one GPU); -2 and -1 are not, and the error says which"""
    from urh_amd import _lib
    g = gold["pad"]
    got, err = run(g, demod("pad"), [0, 300, len(g["iq"])], [1])
    assert not any(err), err
    pieces, p = [x[0] for x in got], mc.params(g["meta"])
    for flag, exc, text in ((0, _lib.UrhGpuError, "capacity"), (-2, RuntimeError, "left the rank's shard"), (-1, RuntimeError, "flag -1")):
        ranks = [x[1][1].copy() for x in got]
        ranks[1]["flag"][1] = flag
        with pytest.raises(exc, match=text) as e:
            S.message_data(pieces, ranks, p)
        assert (flag == 0) == isinstance(e.value, _lib.UrhGpuError)
