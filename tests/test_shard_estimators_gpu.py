"""ShardedPipeline.detect_noise_level / detect_center / iq_to_bits(auto_center=True) on the GPU: W ranks as threads on the one GPU, one
GpuShardEngine each, ThreadComm.  The kernels' records equal the model's (tests/model_shard_estimators.py) bit for bit, the sums equal
np.add.reduce, the estimates equal the single-GPU functions on the whole signal and the oracle."""
from dataclasses import replace

import numpy as np
import pytest

import model_shard_estimators as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline()


@pytest.fixture(scope="module")
def engines():
    from urh_amd.shard_engine import GpuShardEngine
    return [GpuShardEngine(0) for _ in range(8)]


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- urhgpu_pairwise_partial_f32_dev + the combiner ------------------------------------------------------------------------------
def sequence(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)


@pytest.mark.parametrize("n", M.COMBINER_LENGTHS)
def test_pairwise_partial_records_and_combiner(pipe, engines, n):
    import ctypes as C
    from urh_amd import _lib, sharding as S
    x = sequence(n, n)
    dev = cuda(x)
    mean = np.float32(np.add.reduce(x) / np.float32(n))
    want = {0: np.add.reduce(x), 1: np.add.reduce((x - mean) ** 2)}
    e = engines[0]
    for mode in (0, 1):                                     # the single-GPU primitive gives numpy's sum as well
        s = C.c_float(0.0)
        _lib.check(_lib.load().urhgpu_pairwise_sum_f32_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), n, mode, float(mean), C.byref(s)))
        assert same_bits(s.value, want[mode])
    for cuts in M.cut_lists(np.random.default_rng(n + 1), n):
        words = max(S.pairwise_record_words(a, b - a, n) for a, b in cuts)
        for mode in (0, 1):
            recs = np.stack([e.pairwise_partial(dev[a:b], a, n, mode, float(mean), words).cpu().numpy() for a, b in cuts])
            model = np.stack([M.partial_record(x[a:b], a, n, mode, mean, words) for a, b in cuts])
            assert np.array_equal(recs.view(np.uint32), model.view(np.uint32)), (n, cuts, mode, np.nonzero(recs.view(np.uint32) != model.view(np.uint32)))
            got = S.pairwise_combine(recs, n)
            assert same_bits(got, want[mode]), (n, cuts, mode, got, want[mode])
            assert S.minmax_combine(recs) == (float(x.min()), float(x.max()))


def test_pairwise_partial_refuses_a_short_buffer(engines):
    from urh_amd import _lib
    dev = cuda(sequence(20_000, 1))
    with pytest.raises(_lib.UrhGpuError):
        engines[0].pairwise_partial(dev, 0, 20_000, 0, 0.0, 521)       # two full pieces inside: 522 words


# ---- detect_noise_level ------------------------------------------------------------------------------------------------------------
def sharded(engines, world, call, timeout=120):
    """call(ShardedPipeline, rank) on `world` threads -> (results, exceptions)"""
    from urh_amd.sharding import ShardedPipeline
    return M.run_ranks(world, lambda r, comm: call(ShardedPipeline(engines[r], comm), r), timeout)


NOISE_SIZES = (6400, 100_003, 262_144 + 64)


@pytest.fixture(scope="module")
def noise_inputs(oracle):
    """per (dtype, n): the capture, on the host and on the GPU, and the oracle's answer -- computed once"""
    cache = {}

    def get(dtype, n):
        key = (np.dtype(dtype).name, n)
        if key not in cache:
            x = M.bursty_capture(n, n % 1000 + np.dtype(dtype).itemsize, dtype)
            cache[key] = (x, cuda(x), oracle.detect_noise_level(oracle.get_magnitudes(x)))
        return cache[key]
    return get


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", NOISE_SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.int8, np.uint8, np.int16, np.uint16])
def test_noise_level_equals_oracle(pipe, engines, noise_inputs, dtype, n, world):
    from urh_amd.estimators import detect_noise_level_dev
    from urh_amd.sharding import shard_bounds
    x, dev, want = noise_inputs(dtype, n)
    assert want > 0
    bounds = shard_bounds(n, world)
    got, err = sharded(engines, world, lambda sp, r: sp.detect_noise_level(dev[bounds[r][0]:bounds[r][1]], pos_base=bounds[r][0], n_total=n))
    assert not any(err), err
    assert all(g == want for g in got), (got, want)
    if world == 1:
        assert got[0] == detect_noise_level_dev(pipe, dev)


def test_noise_level_straddling_chunks_and_nan(engines, oracle):
    """chunks 0 and 1 cut by shard boundaries, a shard inside one chunk; a uint16 capture with a 65535 + 65535 j sample (its magnitude
    is NaN): the partials carry it as k_mag_chunk_partials does"""
    n = 6400
    x = M.bursty_capture(n, 9)[::-1].copy()
    dev = cuda(x)
    want = oracle.detect_noise_level(oracle.get_magnitudes(x))
    assert want > 0
    for bounds in ([(0, 6300), (6300, 6370), (6370, n)], [(0, 6300), (6300, 6310), (6310, 6399), (6399, n)]):
        got, err = sharded(engines, len(bounds), lambda sp, r: sp.detect_noise_level(dev[bounds[r][0]:bounds[r][1]], pos_base=bounds[r][0], n_total=n))
        assert not any(err) and all(g == want for g in got), (bounds, got, want, err)
    x = M.bursty_capture(n, 11, np.uint16)
    x[n - 40] = 65535
    dev = cuda(x)
    mags = oracle.get_magnitudes(x)
    assert np.isnan(mags[n - 40]) and np.isnan(mags).sum() == 1
    want = oracle.detect_noise_level(mags)
    part = engines[0].noise_partials(dev[3200:], 3200, n, 64, 100).cpu().numpy()
    model = M.ModelEstimatorEngine().noise_partials(x[3200:], 3200, n, 64, 100).numpy()
    assert np.isnan(part[:, 0]).all() and not part[:, 50:].any() and np.array_equal(part[1], model[1], equal_nan=True)
    assert np.allclose(part[0, 1:], model[0, 1:], rtol=1e-12, atol=0)       # fp64 sums of 64 terms in two orders: within 64 x 2^-53
    bounds = [(0, 3200), (3200, n)]
    got, err = sharded(engines, 2, lambda sp, r: sp.detect_noise_level(dev[bounds[r][0]:bounds[r][1]], pos_base=bounds[r][0], n_total=n))
    assert not any(err) and all(g == want for g in got), (got, want, err)


# ---- detect_center ---------------------------------------------------------------------------------------------------------------
def with_noise_runs(kept, seed):
    """the kept samples with runs of -4 of random length inserted: a demodulated signal whose compaction is `kept`"""
    rng = np.random.default_rng(seed)
    pieces, at = [], 0
    while at < len(kept):
        ln = int(rng.integers(200, 3000))
        pieces.append(kept[at:at + ln])
        pieces.append(np.full(int(rng.integers(1, 1500)), -4.0, np.float32))
        at += ln
    return np.concatenate(pieces)


def kept_for_m(m):
    """K with int(0.95 K) - int(0.05 K) == m"""
    for k in range(int(m / 0.9) - 4, int(m / 0.9) + 5):
        if int(0.95 * k) - int(0.05 * k) == m:
            return k
    raise AssertionError(m)


def at_kept(x, k):
    """index in x of its k-th kept sample"""
    return int(np.nonzero(x > -4)[0][k])


def equal_bounds(n, world):
    return M.bounds_for(n, world)


def center_cases():
    """name -> (signal, bounds, max_size)"""
    cases = {}
    for world, n in ((2, 20_000), (3, 120_000), (8, 300_000)):
        cases[f"seeded_w{world}"] = (M.two_level(n, world), equal_bounds(n, world), None)
    x = M.two_level(100_000, 31)
    cases["a_inside_rank0"] = (x, equal_bounds(len(x), 3), None)
    cases["a_inside_rank1"] = (x, [(0, 2_000), (2_000, 60_000), (60_000, len(x))], None)       # rank 0 holds less than 5 % of the kept samples
    y = x.copy()
    y[40_000:70_000] = -4.0
    cases["rank_keeps_nothing"] = (y, [(0, 40_000), (40_000, 70_000), (70_000, len(y))], None)
    y = y.copy()
    y[50_000:50_100] = 0.7
    cases["rank_keeps_fewer_than_128"] = (y, [(0, 40_000), (40_000, 70_000), (70_000, len(y))], None)
    for name, m in (("m_8192j", 3 * 8192), ("m_8192j_plus1", 3 * 8192 + 1), ("m_8192j_minus1", 3 * 8192 - 1)):
        kept = M.two_level(kept_for_m(m), m, noise_runs=False)
        z = with_noise_runs(kept, m)
        cases[name] = (z, equal_bounds(len(z), 3), None)
    kept = M.two_level(50_000, 41, noise_runs=False)
    z = with_noise_runs(kept, 41)
    a = int(0.05 * len(kept))
    c1, c2 = at_kept(z, a + 128 * 70), at_kept(z, a + 8192 * 3)                                  # S's boundaries at a multiple of 128 and of 8192
    cases["boundary_at_multiple_of_128"] = (z, [(0, c1), (c1, c2), (c2, len(z))], None)
    cases["max_size_inside_rank0"] = (x, equal_bounds(len(x), 3), 9_000)
    cases["max_size_larger_than_m"] = (x, equal_bounds(len(x), 3), 10 * len(x))
    w = M.two_level(60_000, 51, noise_runs=False)
    cases["ask_style_nothing_filtered"] = (np.abs(w), equal_bounds(len(w), 8), None)
    cases["constant_signal"] = (np.full(30_000, 0.25, np.float32), equal_bounds(30_000, 3), None)
    return cases


CENTER_CASES = ("seeded_w2", "seeded_w3", "seeded_w8", "a_inside_rank0", "a_inside_rank1", "rank_keeps_nothing", "rank_keeps_fewer_than_128",
                "m_8192j", "m_8192j_plus1", "m_8192j_minus1", "boundary_at_multiple_of_128", "max_size_inside_rank0", "max_size_larger_than_m",
                "ask_style_nothing_filtered", "constant_signal")


@pytest.fixture(scope="module")
def center_inputs():
    cases = center_cases()
    assert sorted(cases) == sorted(CENTER_CASES)
    return cases


@pytest.mark.parametrize("name", CENTER_CASES)
def test_center_equals_single_gpu_and_oracle(pipe, engines, oracle, center_inputs, name):
    from urh_amd.estimators import detect_center_dev
    from urh_amd.sharding import center_parts
    x, bounds, max_size = center_inputs[name]
    dev = cuda(x)
    single = detect_center_dev(pipe, dev, max_size, _single=True)
    want = oracle.detect_center(x, max_size)
    got, err = sharded(engines, len(bounds), lambda sp, r: sp.detect_center(dev[bounds[r][0]:bounds[r][1]], max_size))
    assert not any(err), err
    for g in got:
        assert (g is None) == (single is None) == (want is None), (got, single, want)
        assert g is None or (np.float64(g) == np.float64(single) == np.float64(want)), (got, single, want)
    # the case is what its name says
    m, parts = center_parts([int((x[a:b] > -4).sum()) for a, b in bounds], max_size)
    a_cut = int(0.05 * int((x > -4).sum()))
    kept0 = int((x[:bounds[0][1]] > -4).sum())
    checks = {"a_inside_rank0": a_cut < kept0, "a_inside_rank1": a_cut >= kept0 and parts[0][2] == 0 and parts[1][2] > 0,
              "rank_keeps_nothing": parts[1][2] == 0, "rank_keeps_fewer_than_128": 0 < parts[1][2] < 128,
              "m_8192j": m == 3 * 8192, "m_8192j_plus1": m == 3 * 8192 + 1, "m_8192j_minus1": m == 3 * 8192 - 1,
              "boundary_at_multiple_of_128": parts[1][1] % 128 == 0 and parts[1][1] % 8192 != 0 and parts[2][1] % 8192 == 0 and parts[2][2] > 0,
              "max_size_inside_rank0": m == max_size and parts[0][2] == m and parts[1][2] == 0,
              "max_size_larger_than_m": max_size is not None and m < max_size,
              "ask_style_nothing_filtered": int((x > -4).sum()) == len(x), "constant_signal": want is None}
    assert checks.get(name, True), (name, m, parts)
    if name != "constant_signal":
        assert want is not None


def test_center_golden_psk4_clean(pipe, engines, oracle):
    """the golden 4-PSK capture: its demodulated signal from the single-GPU pass, sharded over 2 and 3 ranks"""
    from conftest import load_golden
    from urh_amd.estimators import detect_center_dev
    from urh_amd.pipeline import DemodParams
    g = load_golden("psk4_clean")
    p = DemodParams("PSK", g["bits_per_symbol"], g["noise_threshold"], g["center"], g["center_spacing"], g["tolerance"], g["samples_per_symbol"],
                    g["costas_loop_bandwidth"], g["pause_threshold"], True)
    qad = pipe.iq_to_bits(cuda(g["iq"]), p, want_qad=True).qad.clone()
    host = qad.cpu().numpy()
    single, want = detect_center_dev(pipe, qad, _single=True), oracle.detect_center(host)
    for bounds in ([(0, 900), (900, 1800)], [(0, 100), (100, 1000), (1000, 1800)]):
        got, err = sharded(engines, len(bounds), lambda sp, r: sp.detect_center(qad[bounds[r][0]:bounds[r][1]]))
        assert not any(err), err
        for v in got:
            assert (v is None) == (single is None) == (want is None)
            assert v is None or np.float64(v) == np.float64(single) == np.float64(want)


# ---- the PSK pass with auto_center -----------------------------------------------------------------------------------------------------
def psk_capture(n, order, seed, offset=0.04):
    """seeded PSK at 100 samples per symbol, carrier offset `offset` cycles per sample, AWGN (as tests/test_costas_shard.py)"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, order, n // 100 + 1)
    phases = (np.array([-135, -45, 45, 135]) if order == 4 else np.array([-90, 90]))[sym] * np.pi / 180
    ph = np.repeat(phases, 100)[:n] + 2 * np.pi * offset * np.arange(n)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1) + 0.1 * np.sqrt(0.5) * rng.standard_normal((n, 2))
    return iq.astype(np.float32), 0.2


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("world", [2, 8])
def test_psk_pass_with_auto_center(pipe, engines, order, world):
    from urh_amd.estimators import detect_center_dev
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import costas_halo_samples, shard_bounds, stitch
    n = 240_000
    iq, noise = psk_capture(n, order, seed=10 * world + order)
    p = DemodParams("PSK", 2 if order == 4 else 1, noise, 0.3, 1.5 if order == 4 else 1.0, 5, 100, 0.1, 8, True)
    dev = cuda(iq)
    center = detect_center_dev(pipe, pipe.iq_to_bits(dev, p, want_qad=True).qad.clone(), _single=True)
    assert center is not None and float(center) != p.center
    single = pipe.iq_to_bits(dev, replace(p, center=float(center)), want_qad=True)
    want = (single.ppseq().copy(),) + tuple(x.copy() for x in single.flat())
    bounds = shard_bounds(n, world)
    halos = [None] + [dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a] for a, _ in bounds[1:]]

    def work(sp, r):
        res = sp.iq_to_bits(dev[bounds[r][0]:bounds[r][1]], p, want_qad=True, pos_base=bounds[r][0], n_total=n, left_raw=halos[r], auto_center=True)
        return res, sp.last_center
    out, err = sharded(engines, world, work, timeout=300)
    assert not any(err), err
    assert all(c == float(center) for _, c in out), ([c for _, c in out], center)
    for k, (a, b) in enumerate(zip(stitch([res for res, _ in out]), want)):
        assert np.array_equal(a, b), (k, len(a), len(b))


# ---- refusals return and do not hang ---------------------------------------------------------------------------------------------------
def test_auto_center_with_fsk_raises_on_every_rank(engines):
    from urh_amd.pipeline import DemodParams
    iq = cuda(M.bursty_capture(20_000, 1))
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, True)
    _, err = sharded(engines, 2, lambda sp, r: sp.iq_to_bits(iq[10_000 * r:10_000 * (r + 1)], p, auto_center=True), timeout=60)
    assert all(isinstance(e, ValueError) and "auto_center" in str(e) for e in err), err


def test_non_contiguous_shard_on_one_rank_raises_and_does_not_hang(engines):
    """the rank whose shard is a strided view raises before it enters a collective; the other leaves its own (broken barrier)"""
    qad = cuda(M.two_level(40_000, 3))
    _, err = sharded(engines, 2, lambda sp, r: sp.detect_center(qad[:20_000] if r == 0 else qad[20_000::2]), timeout=60)
    assert isinstance(err[1], ValueError) and "contiguous" in str(err[1]) and err[0] is not None, err
    iq = cuda(M.bursty_capture(40_000, 4))
    _, err = sharded(engines, 2, lambda sp, r: sp.detect_noise_level(iq[:20_000] if r == 0 else iq[20_000::2], pos_base=20_000 * r, n_total=40_000), timeout=60)
    assert isinstance(err[1], ValueError) and err[0] is not None, err
