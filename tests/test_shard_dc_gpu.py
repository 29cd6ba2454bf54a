"""ShardedPipeline.dc_correct on the GPU: W ranks as threads on the one GPU, one GpuShardEngine each, ThreadComm.  Every case holds the
stitched shards against numpy's own x - np.mean(x, axis=0) on the host, against filter.dc_correct_dev on the whole capture, and the
recorded mean against both; the committed captures of tests/golden/dc/ against the reference's recorded outputs."""
import os

import numpy as np
import pytest

import dc_cases
import model_shard_estimators as M
from conftest import GOLDEN_DIR, synth_fsk
from dc_cases import numpy_dc, same_bits

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


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def equal_cuts(n, world):
    per = -(-n // world)
    return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(world)]


def sharded(engines, world, call, timeout=120):
    from urh_amd.sharding import ShardedPipeline
    return M.run_ranks(world, lambda r, comm: call(ShardedPipeline(engines[r], comm), r), timeout)


@pytest.fixture(scope="module")
def whole(pipe):
    """per input (by id): numpy's result on the host and the single-GPU function's on the whole capture -- computed once"""
    from urh_amd.filter import dc_correct_dev
    cache = {}

    def get(key, x):
        if key not in cache:
            want, want_mean = numpy_dc(x)
            dev = cuda(x)
            out, mean = dc_correct_dev(pipe, dev, want_mean=True)
            cache[key] = (dev, want, want_mean.astype(np.float32 if x.dtype == np.float32 else np.float64), out.cpu().numpy(), mean.cpu().numpy())
        return cache[key]
    return get


def check(engines, whole, key, x, cuts, in_place=False):
    n, world = len(x), len(cuts)
    dev, want, want_mean, single, single_mean = whole(key, x)
    assert same_bits(single, want) and same_bits(single_mean, want_mean)

    def work(sp, r):
        a, b = cuts[r]
        shard = dev[a:b].clone() if in_place else dev[a:b]
        res = sp.dc_correct(shard, pos_base=a, n_total=n, out=shard if in_place else None)
        assert not in_place or res is shard
        return res.cpu().numpy(), sp.last_dc
    got, err = sharded(engines, world, work)
    assert not any(err), err
    out = np.concatenate([g[0] for g in got])
    assert same_bits(out, want), (key, cuts, np.nonzero(out != want)[0][:4])
    assert same_bits(out, single), (key, cuts)
    assert same_bits(dev.cpu().numpy(), x), "the caller's capture was modified"
    for _, dc in got:
        assert same_bits(dc["mean"], want_mean) and same_bits(dc["mean"], single_mean), (key, cuts, dc["mean"], want_mean)
        assert dc["all_gathers"] == got[0][1]["all_gathers"] <= world + 1, (key, cuts, dc)
        assert dc["all_gathers"] >= (1 if x.dtype != np.float32 else 2) or world == 1
    return [dc for _, dc in got]


@pytest.mark.parametrize("n", [30_000, 70_000])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_sample_types_equal_cuts(engines, whole, dtype, n):
    x = dc_cases.generic(dtype, n)
    for world in (1, 2, 3, 8):
        dcs = check(engines, whole, ("generic", np.dtype(dtype).name, n), x, equal_cuts(n, world))
        if world == 1:
            assert dcs[0]["all_gathers"] == 0


UNEVEN = {
    "odd_pos_base": [(0, 10_001), (10_001, 27_777), (27_777, 50_000)],
    "empty_rank": [(0, 20_001), (20_001, 20_001), (20_001, 50_000)],
    "ranks_of_1_and_5": [(0, 9_001), (9_001, 9_002), (9_002, 9_007), (9_007, 50_000)],
    "short_beside_long": [(0, 8_192), (8_192, 12_289), (12_289, 50_000)],
    "nothing_on_rank_0": [(0, 0), (0, 49_997), (49_997, 50_000)],
}


@pytest.mark.parametrize("cuts", sorted(UNEVEN))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_uneven_cuts(engines, whole, dtype, cuts):
    """shards that start off a 16-byte boundary for every sample type, an empty rank, ranks of 1 and 5 samples, a rank of at most 8192
    samples beside one of more"""
    x = dc_cases.generic(dtype, 50_000)
    assert all(a % 2 == 1 for a, _ in UNEVEN["odd_pos_base"][1:])
    check(engines, whole, ("generic", np.dtype(dtype).name, 50_000), x, UNEVEN[cuts])


F32_NAMES = ("zero_mean", "zero_mean_spiked", "nan_mid", "nan_seam", "inf_mid", "inf_minf_seam", "overflow", "sign_change", "ties_odd_k", "odd_guess_ties",
             "denormal_dc", "neg_zero")


@pytest.mark.parametrize("name", F32_NAMES)
def test_float32_cases(engines, whole, name):
    n = 40_001
    x = dc_cases.f32_case(name, n)[0]
    for cuts in (equal_cuts(n, 2), [(0, 12_289), (12_289, 12_290), (12_290, 30_001), (30_001, n)], equal_cuts(n, 8)):
        dcs = check(engines, whole, (name, n), x, cuts)
        if name == "zero_mean_spiked" and len(cuts) != 4:
            # every shard holds a chunk whose path runs up to 2^24 and back (no record of it can be translated: room 0), and the true entry
            # of rank r > 0 is minus / plus the number of chunks in front while its guess is 0: every rank behind the first hands over
            assert dcs[0]["all_gathers"] == len(cuts) + 1 and all(dc["reevaluated"] > 0 for dc in dcs), dcs


def test_zero_mean_noise_and_amplitudes(engines, whole):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((70_000, 2)).astype(np.float32)
    check(engines, whole, "zero_mean_noise", x, equal_cuts(len(x), 3))
    y = (rng.standard_normal((70_000, 2)) * np.exp(rng.uniform(-20, 20, (70_000, 1)))).astype(np.float32)
    check(engines, whole, "amplitudes", y, [(0, 5), (5, 33_333), (33_333, 70_000)])
    check(engines, whole, "amplitudes", y, equal_cuts(len(y), 8))


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.uint8], ids=lambda d: np.dtype(d).name)
def test_in_place(engines, whole, dtype):
    x = dc_cases.generic(dtype, 30_000)
    check(engines, whole, ("generic", np.dtype(dtype).name, 30_000), x, [(0, 10_001), (10_001, 30_000)], in_place=True)


def test_two_ranks_finish_with_two_all_gathers(engines, whole):
    x = (0.5 + 0.1 * np.random.default_rng(1).standard_normal((30_000, 2))).astype(np.float32)
    dcs = check(engines, whole, "two_ranks", x, [(0, 20_000), (20_000, 30_000)])
    assert [dc["all_gathers"] for dc in dcs] == [2, 2], dcs
    assert dcs[1]["chunks"] == 3 and dcs[1]["reevaluated"] == 0 and dcs[1]["derived"] == 12, dcs


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN_DIR, "dc")) if f.endswith(".npz")))
def test_golden_captures_equal_the_reference(engines, whole, name):
    z = np.load(os.path.join(GOLDEN_DIR, "dc", name + ".npz"), allow_pickle=False)
    x, n = z["iq"], len(z["iq"])
    assert same_bits(numpy_dc(x)[0], z["work"])
    for cuts in (equal_cuts(n, 2), [(0, n // 5 | 1), (n // 5 | 1, n // 2 | 1), (n // 2 | 1, n)]):
        check(engines, whole, ("golden", name), x, cuts)


# ---- end to end: dc_correct, then iq_to_bits on the result -----------------------------------------------------------------------------
def single_pass(pipe, dev, p):
    res = pipe.iq_to_bits(dev, p, want_qad=True, dc_correction=True)
    return (res.ppseq().copy(),) + tuple(v.copy() for v in res.flat()), res.qad.cpu().numpy().copy()


def assert_stitched(out, want, want_qad):
    from urh_amd.sharding import stitch
    for k, (a, b) in enumerate(zip(stitch([res for res, _ in out]), want)):
        assert np.array_equal(a, b), (k, len(a), len(b))
    assert same_bits(np.concatenate([q for _, q in out]), want_qad)
    assert len(want[0]) > 10


@pytest.mark.parametrize("halo_given", [False, True])
def test_fsk_pass_on_corrected_shards(pipe, engines, halo_given):
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import shard_bounds
    n, world = 120_000, 3
    iq = synth_fsk(n, sps=50, seed=17, noise=0.02, pause_every=3000, pause_len=1500) * np.float32(0.5) + np.float32(0.3)
    p = DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 50, 0.1, 8, True)
    dev = cuda(iq)
    want, want_qad = single_pass(pipe, dev, p)
    bounds = shard_bounds(n, world)

    def work(sp, r):
        a, b = bounds[r]
        if halo_given and r > 0:
            shard, (halo,) = sp.dc_correct(dev[a:b], pos_base=a, n_total=n, also=(dev[a - 2:a],))
        else:
            shard, halo = sp.dc_correct(dev[a:b], pos_base=a, n_total=n), None
        res = sp.iq_to_bits(shard, p, want_qad=True, pos_base=a, n_total=n, halo_given=halo_given, left_halo=halo)
        return res.piece(), res.qad.cpu().numpy().copy()
    out, err = sharded(engines, world, work)
    assert not any(err), err
    assert_stitched(out, want, want_qad)


def test_psk_pass_on_corrected_shards(pipe, engines):
    from test_shard_estimators_gpu import psk_capture
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import costas_halo_samples, shard_bounds
    n, world = 240_000, 2
    iq, noise = psk_capture(n, 2, seed=22)
    iq = iq + np.array([0.2, -0.1], np.float32)
    p = DemodParams("PSK", 1, noise, 0.0, 1.0, 5, 100, 0.1, 8, True)
    dev = cuda(iq)
    want, want_qad = single_pass(pipe, dev, p)
    bounds = shard_bounds(n, world)

    def work(sp, r):
        a, b = bounds[r]
        if r > 0:
            shard, (left_raw,) = sp.dc_correct(dev[a:b], pos_base=a, n_total=n, also=(dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a],))
        else:
            shard, left_raw = sp.dc_correct(dev[a:b], pos_base=a, n_total=n), None
        res = sp.iq_to_bits(shard, p, want_qad=True, pos_base=a, n_total=n, left_raw=left_raw)
        return res.piece(), res.qad.cpu().numpy().copy()
    out, err = sharded(engines, world, work, timeout=300)
    assert not any(err), err
    assert_stitched(out, want, want_qad)


# ---- refusals return and do not hang ---------------------------------------------------------------------------------------------------
def test_strided_shard_on_one_rank_raises_and_does_not_hang(engines):
    iq = cuda(dc_cases.generic(np.float32, 40_000))
    _, err = sharded(engines, 2, lambda sp, r: sp.dc_correct(iq[:20_000] if r == 0 else iq[20_000::2], pos_base=20_000 * r, n_total=30_000), timeout=60)
    assert isinstance(err[1], ValueError) and "contiguous" in str(err[1]) and err[0] is not None, err


def test_refusals_of_the_entry_points(engines):
    import ctypes as C
    import torch
    from urh_amd import _lib
    lib, e = _lib.load(), engines[0]
    t = torch.zeros((64, 2), dtype=torch.float32, device=e.device)
    words = torch.zeros(8, dtype=torch.int64, device=e.device)
    h, p, w = e.ctx.handle, C.c_void_p(t.data_ptr()), C.c_void_p(words.data_ptr())
    assert lib.urhgpu_shard_dc_sums_dev(h, p, 64, 7, w) == _lib.ERR_DTYPE
    assert lib.urhgpu_shard_dc_sums_dev(h, C.c_void_p(t.data_ptr() + 4), 8, _lib.DT_F32, w) == _lib.ERR_ARG            # half a sample
    assert lib.urhgpu_shard_dc_spec_dev(h, p, 64, (C.c_double * 2)(0.0, 0.0), w) == _lib.OK
    assert lib.urhgpu_shard_dc_resolve_dev(h, p, 32, (C.c_uint32 * 2)(0, 0), w) == _lib.ERR_ARG                         # not the shard last speculated
    assert lib.urhgpu_shard_dc_apply_dev(h, p, 8, _lib.DT_F32, (C.c_float * 2)(0.0, 0.0), C.c_void_p(t.data_ptr() + 8)) == _lib.ERR_ARG   # overlap
    with pytest.raises(ValueError, match="also"):
        e.dc_own(t, (t.to(torch.int16),), None)
    with pytest.raises(ValueError, match="lies on"):
        e.dc_own(t.cpu(), (), None)
    e.ctx.sync()
