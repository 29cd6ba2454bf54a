"""ShardedPipeline.message_records on the GPU: W ranks as threads on the one GPU, one GpuShardEngine each, ThreadComm (the pass, then the
records on the same shard).  The committed fixtures of tests/golden/msg_records/ at the boundary sets of tests/shard_record_cases.py against
what the REAL reference recorded and against DevicePipeline.iq_to_bits(msg_records=True) on the whole capture; synthetic captures of all
five sample types, a PSK pass, a pass on DC-corrected shards and a rank that exceeds a capacity against the single-GPU records.  Records
are compared field by field, the RSSI on its bytes."""
import numpy as np
import pytest

import model_shard_estimators as M
import msg_record_cases as mc
import shard_record_cases as sc
from conftest import synth_fsk

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.float32]


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def engines():
    from urh_amd.shard_engine import GpuShardEngine
    return [GpuShardEngine(0) for _ in range(8)]


@pytest.fixture(scope="module")
def gold():
    return mc.load()


def to_dev(iq):
    import torch
    a = np.ascontiguousarray(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def single_records(pipe, dev, p, divisor, **kw):
    """the single-GPU pass on the whole capture: (records, the list of MessageData)"""
    res = pipe.iq_to_bits(dev, p, want_qad=True, msg_records=True, message_length_divisor=divisor, **kw)
    return res.records.copy(), res.message_data()


def run(engines, dev, edges, p, divisors, halos=None, before=None, timeout=120):
    """the pass and, for every divisor, the records on len(edges) - 1 ranks -> per rank (result, {divisor: records}, {divisor: last_records});
    shards are cloned slices: the pass wants a 16-byte-aligned shard pointer and the cuts fall at arbitrary samples"""
    from urh_amd.sharding import ShardedPipeline
    n, world = edges[-1], len(edges) - 1

    def work(r, comm):
        sp = ShardedPipeline(engines[r], comm)
        a, b = edges[r], edges[r + 1]
        shard, kw = dev[a:b].clone(), {}
        if before is not None:
            shard, kw = before(sp, r, shard, a)
        elif halos is not None:
            kw = dict(left_raw=halos[r])
        res = sp.iq_to_bits(shard, p, want_qad=True, pos_base=a, n_total=n, **kw)
        recs, last = {}, {}
        for d in divisors:
            recs[d] = sp.message_records(shard, res, p, d, pos_base=a, n_total=n)
            last[d] = sp.last_records
        return res, recs, last
    got, err = M.run_ranks(world, work, timeout)
    assert not any(err), (edges, err)
    return got


def check_against_single(got, edges, p, divisor, want_rec, want_msgs, what):
    """stitched records == the single-GPU records, messages == the single-GPU messages, and the protocol's counts"""
    from urh_amd import sharding as S
    ranks = [x[1][divisor] for x in got]
    rec = S.stitch_records(ranks)
    sc.assert_same_records(rec, want_rec, what)
    msgs = S.message_data([x[0] for x in got], ranks, p)
    assert [(list(a.plain_bits), a.pause, list(a.bit_sample_pos), a.timestamp) for a in msgs] == \
           [(list(a.plain_bits), a.pause, list(a.bit_sample_pos), a.timestamp) for a in want_msgs], what
    assert all(mc.same_float(a.rssi, b.rssi) for a, b in zip(msgs, want_msgs)), what
    world = len(edges) - 1
    outside, later = sc.outside_windows(want_rec, [len(r) for r in ranks], edges, int(p.samples_per_symbol))
    assert not later, (what, later)
    lasts = [x[2][divisor] for x in got]
    assert all(l == lasts[0] for l in lasts), (what, lasts)
    assert lasts[0]["windows"] == len(outside), (what, lasts[0], outside)
    assert lasts[0]["all_gathers"] == (0 if world == 1 else 3 if outside else 2), (what, lasts[0])
    return msgs, len(outside)


# ---- 1. the committed fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.names())
def test_fixtures_at_every_boundary_set(pipe, engines, gold, case):
    g = gold[case]
    m = g["meta"]
    p, dev = mc.params(m), to_dev(g["iq"])
    divisors = [int(d) for d in m["divisors"]]
    single = {d: single_records(pipe, dev, p, d) for d in divisors}
    n_msg = len(g["want"][1]["pauses"])
    sets = sc.boundary_sets(case, g, 1, n_random=1)
    for d in divisors:
        if d > 1:
            sets.update({f"d{d}:{k}": v for k, v in sc.targeted_edges(g, d).items() if "pad" in k})
    if n_msg > 500:
        # 1500 records per divisor and set, and every GPU test takes a few seconds at the most: of the per-message targeted cuts every
        # third one (the host file runs them all); the one-rank, equal and random cuts all stay
        general = {k: v for k, v in sets.items() if ":" not in k}
        targeted = [k for k in sets if ":" in k]
        sets = {**general, **{k: sets[k] for k in targeted[::3]}}
        assert any(k.endswith(":mid") for k in sets) and len(sets) >= len(general) + len(targeted) // 3
    if len(g["iq"]) >= 16:
        assert {"one-rank", "equal-2", "equal-3", "equal-8"} <= set(sets) and all(f"random-{w}-0" in sets for w in (2, 3, 4, 8)), sorted(sets)
    for name, edges in sets.items():
        got = run(engines, dev, edges, p, divisors)
        for d in divisors:
            what = (case, d, name, edges)
            msgs, _ = check_against_single(got, edges, p, d, single[d][0], single[d][1], what)
            from urh_amd import sharding as S
            msgs = S.message_data([x[0] for x in got], [x[1][d] for x in got], p, m["sample_rate"], m["timestamp"])
            mc.assert_messages(msgs, g["want"][d], what)                           # what the REAL reference recorded
            sc.assert_same_records(S.stitch_records([x[1][d] for x in got]), sc.whole_records(g, d), what)


def test_a_window_over_eight_ranks_is_exchanged(pipe, engines, gold):
    g = gold["w9000-float32"]
    p, dev = mc.params(g["meta"]), to_dev(g["iq"])
    edges = sc.boundary_sets("w9000-float32", g, 1)["window-over-8-ranks"]
    got = run(engines, dev, edges, p, [1])
    rec, msgs = single_records(pipe, dev, p, 1)
    assert check_against_single(got, edges, p, 1, rec, msgs, "w9000")[1] == 1
    assert got[0][2][1] == {"all_gathers": 3, "windows": 1}


# ---- 2. synthetic captures -----------------------------------------------------------------------------------------------------------
def synthetic(dtype, n=60_001, sps=50):
    """FSK bursts between silent gaps in every sample type (unsigned: the bursts ride on half the range and the gaps stay at zero, so that the
    gaps are silent there too) and the noise threshold that gates the gaps"""
    iq = synth_fsk(n, sps=sps, seed=31, noise=0.02, pause_every=2500, pause_len=700, dtype=np.float32) * np.float32(0.6)
    if np.dtype(dtype) == np.float32:
        return iq, 0.2
    info = np.iinfo(dtype)
    if np.dtype(dtype).kind == "u":
        gap = (np.abs(iq) < 0.2).all(axis=1)
        iq = np.abs(np.where(gap[:, None], iq * 0.5, 0.5 + 0.5 * iq))
    return np.clip(np.round(iq * (info.max * 0.9)), info.min, info.max).astype(dtype), 0.2 * info.max * 0.9


@pytest.mark.parametrize("mod", ["FSK", "ASK"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_synthetic_captures_equal_the_single_gpu_records(pipe, engines, dtype, mod):
    from urh_amd.pipeline import DemodParams
    iq, noise = synthetic(dtype)
    n, dev = len(iq), to_dev(iq)
    p = DemodParams(mod, 1, noise, 0.0 if mod == "FSK" else 0.1 * noise, 1.0, 5, 50, 0.1, 8, True)
    divisors = [1, 8]
    single = {d: single_records(pipe, dev, p, d) for d in divisors}
    assert len(single[1][0]) > 10 and (mod != "ASK" or single[8][0]["n_pad"].any())
    mids = single[1][0]["mid_pos"]
    exchanged = 0
    for edges in ([0, n], sc.equal_edges(n, 2), sc.equal_edges(n, 3), sc.equal_edges(n, 8),
                  [0, 20_001, 40_003, n],                                         # odd pos_base values
                  [0, int(mids[3]) + 7, int(mids[9]) + 1, int(mids[9]) + 3, int(mids[9]) + 8, n]):     # boundaries inside two windows
        got = run(engines, dev, edges, p, divisors)
        for d in divisors:
            exchanged += check_against_single(got, edges, p, d, single[d][0], single[d][1], (np.dtype(dtype).name, mod, d, edges))[1]
    assert exchanged >= 2


# ---- 3. PSK, and a pass on DC-corrected shards ----------------------------------------------------------------------------------------
def test_psk_pass(pipe, engines):
    from test_costas_shard import params, psk_capture
    from urh_amd.sharding import costas_halo_samples
    n = 100_000
    iq, noise = psk_capture(n, 2, seed=5, gaps=[(20_000, 23_000), (50_000, 54_000), (80_000, 82_000)])
    p, dev = params(2, noise), to_dev(iq)
    rec, msgs = single_records(pipe, dev, p, 1)
    assert len(rec) >= 3
    edges = [0, int(rec["mid_pos"][1]) + 13, 70_001, n]                           # a boundary inside the second message's window
    halos = [None] + [dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a].clone() for a in edges[1:-1]]
    got = run(engines, dev, edges, p, [1, 8], halos=halos, timeout=300)
    assert check_against_single(got, edges, p, 1, rec, msgs, "psk")[1] >= 1
    check_against_single(got, edges, p, 8, rec, msgs, "psk, divisor 8")          # only ASK is padded


def test_records_on_dc_corrected_shards(pipe, engines):
    from urh_amd.pipeline import DemodParams
    n = 60_000
    iq = synth_fsk(n, sps=50, seed=17, noise=0.02, pause_every=3000, pause_len=1500) * np.float32(0.5) + np.float32(0.3)
    p, dev = DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 50, 0.1, 8, True), to_dev(iq)
    rec, msgs = single_records(pipe, dev, p, 1, dc_correction=True)
    assert len(rec) > 5
    edges = [0, int(rec["mid_pos"][2]) + 20, 40_001, n]

    def before(sp, r, shard, a):
        return sp.dc_correct(shard, pos_base=a, n_total=n), {}
    got = run(engines, dev, edges, p, [1], before=before)
    assert check_against_single(got, edges, p, 1, rec, msgs, "dc")[1] >= 1


def test_records_behind_the_tail_of_a_pipelined_engine(pipe):
    """two passes in a row on pipelined engines (the tail on its own stream), the records of each queued behind its tail"""
    from urh_amd.pipeline import DemodParams
    from urh_amd.shard_engine import GpuShardEngine
    n = 524_288
    iq = synth_fsk(n, sps=50, seed=6, noise=0.05, pause_every=n // 16, pause_len=n // 124)
    p, dev = DemodParams("FSK", 1, 0.2, 0.0, 1.0, 3, 50, 0.1, 8, True), to_dev(iq)
    rec, msgs = single_records(pipe, dev, p, 1)
    assert len(rec) > 8
    piped = [GpuShardEngine(0, pipelined=True) for _ in range(2)]
    exchanged = 0
    for k in (4, 7):
        edges = [0, int(rec["mid_pos"][k]) + 24, n]
        got = run(piped, dev, edges, p, [1])
        exchanged += check_against_single(got, edges, p, 1, rec, msgs, ("pipelined", k))[1]
    assert exchanged == 2


# ---- 4. capacities, refusals ------------------------------------------------------------------------------------------------------------
def test_a_rank_with_too_small_a_bits_capacity(pipe, engines):
    from urh_amd import _lib, sharding as S
    from urh_amd.pipeline import DemodParams
    iq, noise = synthetic(np.float32)
    n, dev = len(iq), to_dev(iq)
    p = DemodParams("FSK", 1, noise, 0.0, 1.0, 5, 50, 0.1, 8, True)
    rec, _ = single_records(pipe, dev, p, 1)
    edges = [0, int(rec["mid_pos"][4]) + 5, int(rec["mid_pos"][8]) + 5, n]
    eng, plain = engines[1], engines[1].capacities
    extra = (n - (edges[2] - edges[1])) // 50 + 1                                 # what the engine adds for rows that span other shards

    def small(n_local, pp, cap_rows=None):
        rows, _, msgs, pos = plain(n_local, pp, cap_rows)
        return rows, 16 - extra, msgs, pos                                        # room for 16 bits
    eng.capacities = small
    try:
        got = run(engines, dev, edges, p, [1])
    finally:
        del eng.capacities
    ranks = [x[1][1] for x in got]
    assert (ranks[0]["flag"] == 1).all() and len(ranks[1]) > 1 and (ranks[1]["flag"] == 0).all()
    assert ranks[2]["flag"][0] == 0 and (ranks[2]["flag"][1:] == 1).all()          # its first message began on the rank that failed
    sc.assert_same_records(ranks[0], rec[:len(ranks[0])], "rank 0")
    sc.assert_same_records(ranks[2][1:], rec[len(rec) - len(ranks[2]) + 1:], "rank 2")
    with pytest.raises(_lib.UrhGpuError):
        S.message_data([x[0] for x in got], ranks, p)
    with pytest.raises(_lib.UrhGpuError):                                           # ... as the single-GPU route does
        pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=64, msg_records=True).message_data()


def test_refusals_of_the_entry_points(engines, gold):
    import ctypes as C
    import torch
    from urh_amd import _lib
    g = gold["pad"]
    p, dev = mc.params(g["meta"]), to_dev(g["iq"])
    n = len(g["iq"])
    (res, _, _), = run(engines[:1], dev, [0, n], p, [1])
    e, lib = engines[0], _lib.load()
    o, cp = e._records_outputs(res), p.to_c(np.float32)
    words = torch.zeros(16, dtype=torch.int64, device=e.device)
    rec = torch.zeros(64 * 32 + 16, dtype=torch.uint8, device=e.device)
    first = (C.c_int64 * 8)()
    h, iq, w, r = e.ctx.handle, C.c_void_p(dev.data_ptr()), C.c_void_p(words.data_ptr()), C.c_void_p(rec.data_ptr())
    assert lib.urhgpu_shard_records_summary_dev(h, n, 0, C.byref(o), C.c_void_p(words.data_ptr() + 4)) == _lib.ERR_ARG      # misaligned
    assert lib.urhgpu_shard_records_lookup_dev(h, C.byref(o), None, 2, w) == _lib.ERR_ARG
    assert lib.urhgpu_shard_msg_records_dev(h, iq, n, 0, n, C.byref(cp), C.byref(o), 0, first, None, 0, r, 64, None) == _lib.ERR_ARG     # divisor
    assert lib.urhgpu_shard_msg_records_dev(h, iq, n, 1, n, C.byref(cp), C.byref(o), 1, first, None, 0, r, 64, None) == _lib.ERR_ARG     # not inside the capture
    assert lib.urhgpu_shard_msg_records_dev(h, iq, n, 0, n, C.byref(cp), C.byref(o), 1, first, None, 0, C.c_void_p(rec.data_ptr() + 8), 64, None) == _lib.ERR_ARG
    assert lib.urhgpu_shard_msg_records_dev(h, iq, n, 0, n, C.byref(cp), C.byref(o), 1, None, None, 0, r, 64, None) == _lib.ERR_ARG      # no descriptor
    bad = p.to_c(np.float32)
    bad.dtype = 7
    assert lib.urhgpu_shard_msg_records_dev(h, iq, n, 0, n, C.byref(bad), C.byref(o), 1, first, None, 0, r, 64, None) == _lib.ERR_DTYPE
    o2 = _lib.Outputs()
    C.memmove(C.byref(o2), C.byref(o), C.sizeof(_lib.Outputs))
    o2.pos = None
    assert lib.urhgpu_shard_records_summary_dev(h, n, 0, C.byref(o2), w) == _lib.ERR_ARG                                     # no positions to read
    assert lib.urhgpu_shard_records_summary_dev(h, n, 0, C.byref(o), w) == 0
    e.ctx.sync()
    assert words[:3].tolist() == [0, n, len(g["want"][1]["pauses"])]


def test_a_window_outside_the_shard_is_flagged_and_not_read(engines, gold):
    """flag -2: the kernel is told that the shard is the capture's first 100 samples while the outputs are the whole capture's -- every
    message whose window leaves those 100 samples gets flag -2 and a NaN, the first one included when no assembled window is given"""
    import ctypes as C
    import torch
    from urh_amd import _lib
    from urh_amd.protocol import RECORD_DTYPE
    g = gold["pad"]
    p, dev, n = mc.params(g["meta"]), to_dev(g["iq"]), len(g["iq"])
    (res, recs, _), = run(engines[:1], dev, [0, n], p, [1])
    whole = recs[1]
    assert (whole["flag"] == 1).all() and (whole["mid_pos"][1:] > 100).all() and whole["mid_pos"][0] + 10 <= 100
    e, lib = engines[0], _lib.load()
    o, cp = e._records_outputs(res), p.to_c(np.float32)
    d_rec = torch.zeros(64 * 32, dtype=torch.uint8, device=e.device)
    args = (e.ctx.handle, C.c_void_p(dev.data_ptr()), 100, 0, n, C.byref(cp), C.byref(o), 1)
    for first_mid, want0 in ((int(whole["mid_pos"][0]), 1), (300, -2)):
        first = (C.c_int64 * 8)(1, 1, 3, 0, int(whole["first_pos"][0]), first_mid, 1, 0)
        assert lib.urhgpu_shard_msg_records_dev(*args, first, None, 0, C.c_void_p(d_rec.data_ptr()), 64, None) == 0
        e.ctx.sync()
        got = d_rec.cpu().numpy().view(RECORD_DTYPE)[:len(whole)]
        assert got["flag"].tolist() == [want0] + [-2] * (len(whole) - 1)
        assert np.isnan(got["rssi"][1:]).all() and np.array_equal(got["mid_pos"][1:], whole["mid_pos"][1:])
        if want0 == 1:
            sc.assert_same_records(got[:1], whole[:1], "first message inside the 100 samples")
        else:
            assert np.isnan(got["rssi"][0])
