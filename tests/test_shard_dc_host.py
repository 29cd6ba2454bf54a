"""ShardedPipeline.dc_correct on the CPU: the orchestration and dc_compose of urh_amd/sharding.py driven by the numpy model of the engine
(tests/model_shard_dc.py) over ThreadComm and a world-size-2 gloo group, against numpy's own x - np.mean(x, axis=0)."""
import os

import numpy as np
import pytest

import dc_cases
import model_dc
import model_shard_dc as MD
import model_shard_estimators as M
from urh_amd import sharding as S


def equal_cuts(n, world):
    per = -(-n // world)
    return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(world)]


def random_cuts(rng, n, world):
    e = [0] + sorted(int(c) for c in rng.integers(0, n + 1, world - 1)) + [n]
    return [(e[r], e[r + 1]) for r in range(world)]


def run(x, cuts, also=None, in_place=False):
    """dc_correct of x cut at `cuts`, one model engine per rank -> (stitched output, the ranks' last_dc, engines, the ranks' also results)"""
    n = len(x)
    engines = [MD.ModelDcEngine() for _ in cuts]

    def work(r, comm):
        a, b = cuts[r]
        sp = S.ShardedPipeline(engines[r], comm)
        shard = x[a:b].copy()
        res = sp.dc_correct(shard, pos_base=a, n_total=n, also=also[r] if also else (), out=shard if in_place else None)
        assert not in_place or (res[0] if isinstance(res, tuple) else res) is shard
        return res, sp.last_dc
    got, err = M.run_ranks(len(cuts), work)
    assert not any(err), err
    pairs = [g[0] if isinstance(g[0], tuple) else (g[0], None) for g in got]
    assert all((p[1] is not None) == bool(also and also[r]) for r, p in enumerate(pairs))
    return np.concatenate([p[0] for p in pairs]), [g[1] for g in got], engines, [p[1] for p in pairs]


def check(x, cuts):
    world = len(cuts)
    out, dcs, _, _ = run(x, cuts)
    if x.dtype == np.float32:
        want, mean = dc_cases.numpy_dc(x)
        mean = mean.astype(np.float32)
    else:
        mean, want = model_dc.dc_correct_int(x)
        ref, ref_mean = dc_cases.numpy_dc(x)
        assert dc_cases.same_bits(want, ref) and dc_cases.same_bits(mean, ref_mean)
    assert dc_cases.same_bits(out, want), (cuts, np.nonzero(out != want)[0][:4])
    for dc in dcs:
        assert dc_cases.same_bits(dc["mean"], mean), (cuts, dc["mean"], mean)
        assert dc["all_gathers"] == dcs[0]["all_gathers"]
        assert (world > 1) <= dc["all_gathers"] <= world + 1 and (world > 1 or dc["all_gathers"] == 0), (cuts, dc)
        assert x.dtype == np.float32 or dc["all_gathers"] == min(world - 1, 1)
    return dcs


def amplitudes(n, seed):
    """amplitudes from e^-20 to e^20: every chunk's sum lives in another binade"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-20, 20, (n, 1)))).astype(np.float32)


F32_INPUTS = {
    "dc_offset": lambda: (0.5 + 0.1 * np.random.default_rng(1).standard_normal((30_000, 2))).astype(np.float32),
    "dc_negative": lambda: dc_cases.F32_CASES["dc_10x_neg"](40_001),
    "zero_mean_noise": lambda: np.random.default_rng(2).standard_normal((30_000, 2)).astype(np.float32),
    "zero_mean_exact": lambda: dc_cases.F32_CASES["zero_mean"](30_000),
    "zero_mean_spiked": lambda: dc_cases.F32_CASES["zero_mean_spiked"](30_000),
    "nan_mid": lambda: dc_cases.F32_CASES["nan_mid"](30_000),
    "inf_seam": lambda: dc_cases.F32_CASES["inf_seam"](30_000),
    "inf_minf_mid": lambda: dc_cases.F32_CASES["inf_minf_mid"](30_000),
    "overflow": lambda: dc_cases.F32_CASES["overflow"](30_000),
    "amplitudes": lambda: amplitudes(30_000, 3),
    "ties_odd_k": lambda: dc_cases.F32_CASES["ties_odd_k"](30_000),
    "odd_guess_ties": lambda: dc_cases.F32_CASES["odd_guess_ties"](30_000),
    "neg_zero": lambda: dc_cases.F32_CASES["neg_zero"](20_000),
}


@pytest.mark.parametrize("name", sorted(F32_INPUTS))
def test_float32_equals_numpy_for_every_cut(name):
    x = F32_INPUTS[name]()
    n = len(x)
    rng = np.random.default_rng(len(name))
    cut_lists = [equal_cuts(n, 2), equal_cuts(n, 8), random_cuts(rng, n, 3), random_cuts(rng, n, int(rng.integers(4, 8))),
                 [(0, 12_000), (12_000, 12_000), (12_000, n)],                       # an empty rank
                 [(0, 9_001), (9_001, 9_002), (9_002, 9_007), (9_007, n)],           # ranks of 1 and 5 samples
                 [(0, 0), (0, n - 3), (n - 3, n)]]                                   # nothing on rank 0
    for cuts in cut_lists:
        dcs = check(x, cuts)
        if name == "zero_mean_spiked" and cuts in cut_lists[:2]:
            # every shard holds a chunk whose path runs up to 2^24 and back (room 0), and the true entry of rank r > 0 is minus / plus the
            # number of chunks in front while its guess is 0: every rank behind the first hands its exit over
            assert dcs[0]["all_gathers"] == len(cuts) + 1, dcs


def test_random_amplitudes_random_cuts():
    rng = np.random.default_rng(7)
    counts = set()
    for k in range(6):
        n = int(rng.integers(9_000, 50_000))
        x = amplitudes(n, 100 + k) if k % 2 else (amplitudes(n, 100 + k) + np.float32(np.exp(rng.uniform(-3, 3))))
        for world in (2, 5, 8):
            counts.add(check(x, random_cuts(rng, n, world))[0]["all_gathers"])
    assert min(counts) >= 2


@pytest.mark.parametrize("dtype", dc_cases.INT_DTYPES)
def test_integers_equal_the_model_and_numpy(dtype):
    x = dc_cases.generic(dtype, 30_001)
    rng = np.random.default_rng(5)
    for cuts in (equal_cuts(len(x), 1), equal_cuts(len(x), 2), random_cuts(rng, len(x), 3), random_cuts(rng, len(x), 8),
                 [(0, 7), (7, 7), (7, 8), (8, len(x))]):
        check(x, cuts)
    for name, y in dc_cases.int_cases().items():
        if y.dtype == dtype:
            check(y, random_cuts(rng, len(y), 3))


def test_one_rank_and_empty_capture_enter_no_collective():
    class NoComm:
        rank, world = 0, 1

        def all_gather(self, t):
            raise AssertionError("a collective")
    x = F32_INPUTS["dc_offset"]()
    sp = S.ShardedPipeline(MD.ModelDcEngine(), NoComm())
    want, mean = dc_cases.numpy_dc(x)
    assert dc_cases.same_bits(sp.dc_correct(x), want) and dc_cases.same_bits(sp.last_dc["mean"], mean.astype(np.float32))
    assert sp.last_dc["all_gathers"] == 0 and sp.last_dc["chunks"] == 8
    NoComm.world = 4
    sp = S.ShardedPipeline(MD.ModelDcEngine(), NoComm())
    empty = np.zeros((0, 2), np.int16)
    assert sp.dc_correct(empty, pos_base=0, n_total=0) is empty and sp.last_dc["all_gathers"] == 0


def test_two_ranks_finish_with_two_all_gathers():
    """rank 1's float64 guess lies a few ulps from its true entry; the record of rank 1 holds for more than 2^16 ulps around it, so the
    count does not turn on the order of a float64 sum"""
    x = (0.5 + 0.1 * np.random.default_rng(1).standard_normal((30_000, 2))).astype(np.float32)
    cuts = [(0, 20_000), (20_000, 30_000)]
    out, dcs, engines, _ = run(x, cuts)
    assert dc_cases.same_bits(out, dc_cases.numpy_dc(x)[0])
    assert [dc["all_gathers"] for dc in dcs] == [2, 2]
    true_entry = np.cumsum(x[:20_000], axis=0, dtype=np.float32)[-1].view(np.uint32).astype(np.int64)
    guess = x[:20_000].astype(np.float64).sum(axis=0).astype(np.float32).view(np.uint32).astype(np.int64)
    assert np.all(np.abs(true_entry - guess) < 64), (true_entry, guess)
    assert int(engines[1].rooms.min()) >= 1 << 16, engines[1].rooms
    assert dcs[1]["chunks"] == 3 and dcs[1]["reevaluated"] == 0


def test_also_tensors_take_the_same_mean():
    x = F32_INPUTS["dc_offset"]()
    want, _ = dc_cases.numpy_dc(x)
    cuts = equal_cuts(len(x), 3)
    also = [(x[max(a - 2, 0):a].copy(), x[max(a - 9, 0):a].copy().view(np.complex64).reshape(-1)) for a, _ in cuts]
    out, _, _, fixed = run(x, cuts, also=also, in_place=True)
    assert dc_cases.same_bits(out, want)
    for (a, _), (halo, raw) in zip(cuts, fixed):
        assert dc_cases.same_bits(halo, want[max(a - 2, 0):a]) and raw.dtype == np.complex64
        assert dc_cases.same_bits(raw.view(np.float32).reshape(-1, 2), want[max(a - 9, 0):a])
    y = dc_cases.generic(np.uint8, 5_000)
    _, want_y = model_dc.dc_correct_int(y)
    out, _, _, fixed = run(y, [(0, 3_000), (3_000, 5_000)], also=[(), (y[2_998:3_000].copy(),)])
    assert dc_cases.same_bits(out, want_y) and dc_cases.same_bits(fixed[1][0], want_y[2_998:3_000])


# ---- dc_compose: a pure function of the gathered records -----------------------------------------------------------------------------
def bits(v):
    return int(np.float32(v).view(np.uint32))


def test_compose_exact_hit_translation_and_pending():
    one, two = bits(1.0), bits(2.0)
    rec = np.zeros((3, 2, 2, 4), np.uint32)
    rec[0, :, 0] = (0, one, 0, 0)                                   # rank 0: from +0.0 to 1.0
    rec[0, :, 1] = (1, one + 1, 0, 0)
    rec[1, :, 0] = (one + 4, two + 4, 6, 0)                         # rank 1 guessed 4 ulps above: translated by -4
    rec[1, :, 1] = (one + 5, two + 5, 6, 0)
    rec[2, :, 0] = (two, two, 0, MD.IDENTITY)                       # an empty rank
    entries, pending, total = S.dc_compose(rec)
    assert pending is None and entries == [(0, 0), (one, one), (two, two)] and total == (two, two)
    rec[1, 1, :, 2] = 2                                             # column Q: the room does not reach
    entries, pending, total = S.dc_compose(rec)
    assert pending == 1 and entries == [(0, 0), (one, one), None] and total is None
    entries, pending, total = S.dc_compose(rec, {1: (two, two + 9)})
    assert pending is None and entries[2] == (two, two + 9) and total == (two, two + 9)
    rec[1, 1, :, 2] = 6
    rec[1, 0, :, 0] |= 0x80000000                                   # column I guessed on the other side of zero
    assert S.dc_compose(rec)[1] == 1
    rec[0, :, 0, 1] = 0x7FC00000                                    # a NaN sum passes through every later rank
    assert S.dc_compose(rec)[1:] == (None, (0x7FC00000, 0x7FC00000))
    odd = np.zeros((2, 2, 2, 4), np.uint32)
    odd[0, :, 0] = (0, one + 3, 0, 0)
    odd[1, :, 0] = (one, two, 100, 0)                               # 3 ulps from path 0: path 1 is the one an even distance away
    odd[1, :, 1] = (one + 1, two + 2, 100, 0)
    assert S.dc_compose(odd)[2] == (two + 4, two + 4)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_sample_counts_that_do_not_add_up_raise_on_every_rank():
    x = F32_INPUTS["dc_offset"]()

    def work(r, comm):
        try:                                # (caught here: a rank that raised out of `work` would break the barrier the others are still leaving)
            return S.ShardedPipeline(MD.ModelDcEngine(), comm).dc_correct(x[10_000 * r:10_000 * (r + 1)], pos_base=10_000 * r, n_total=30_001)
        except ValueError as exc:
            return exc
    got, err = M.run_ranks(3, work, timeout=60)
    assert not any(err) and all(isinstance(e, ValueError) and "30001" in str(e) for e in got), (got, err)


def test_refusals_before_any_collective():
    x = F32_INPUTS["dc_offset"]()

    def work(r, comm):
        also = (x[:2].astype(np.float64),) if r == 1 else ()
        return S.ShardedPipeline(MD.ModelDcEngine(), comm).dc_correct(x[15_000 * r:15_000 * (r + 1)], also=also)
    _, err = M.run_ranks(2, work, timeout=60)
    assert isinstance(err[1], ValueError) and "also" in str(err[1]) and err[0] is not None and not isinstance(err[0], ValueError), err
    sp = S.ShardedPipeline(MD.ModelDcEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="contiguous"):
        sp.dc_correct(x[::2])
    with pytest.raises(ValueError, match="inside the capture"):
        sp.dc_correct(x, pos_base=5, n_total=len(x))
    with pytest.raises(ValueError, match="dtype"):
        sp.dc_correct(x.astype(np.float64))
    with pytest.raises(NotImplementedError):
        S.ShardedPipeline(M.ModelEstimatorEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0)).dc_correct(x)


# ---- the real multi-process path -------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sp = S.ShardedPipeline(MD.ModelDcEngine(), S.TorchDistComm())
        res = []
        for x in (amplitudes(25_000, 9), dc_cases.generic(np.int16, 25_000)):
            a, b = (0, 9_001) if rank == 0 else (9_001, len(x))
            res.append((sp.dc_correct(x[a:b], pos_base=a, n_total=len(x)), sp.last_dc))
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_over_gloo():
    """world_size 2, one process per rank, torch.distributed gloo"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, 31500 + os.getpid() % 2000, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for k, x in enumerate((amplitudes(25_000, 9), dc_cases.generic(np.int16, 25_000))):
        want, mean = dc_cases.numpy_dc(x)
        assert dc_cases.same_bits(np.concatenate([got[0][k][0], got[1][k][0]]), want)
        for r in range(2):
            dc = got[r][k][1]
            assert dc_cases.same_bits(dc["mean"], mean.astype(dc["mean"].dtype)) and 1 <= dc["all_gathers"] <= 3
