"""ShardedPipeline.detect_noise_level / detect_center on the CPU: the orchestration and the record combiner of urh_amd/sharding.py
driven by the numpy model of the engine (tests/model_shard_estimators.py) over ThreadComm, against numpy and the oracle."""
import numpy as np
import pytest

import model_shard_estimators as M
from urh_amd import sharding as S


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---- the combiner: np.add.reduce bit for bit, for every way of cutting the sequence --------------------------------------------------
def sequence(n, seed):
    """float32 values of mixed sign and magnitude: every order of adding them rounds differently"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.uniform(-6, 6, n))).astype(np.float32)


def combine_cut(x, cuts, mode, mean):
    recs = [M.partial_record(x[a:b], a, len(x), mode, mean) for a, b in cuts]
    words = max(len(r) for r in recs)
    assert all(len(r) == S.pairwise_record_words(a, b - a, len(x)) for r, (a, b) in zip(recs, cuts))
    assert all(len(r) <= (b - a) // 8192 + S.PW_REC_PIECES for r, (a, b) in zip(recs, cuts))     # m_local / 8192 + a few hundred floats
    stacked = np.stack([np.concatenate([r, np.zeros(words - len(r), np.float32)]) for r in recs])
    return S.pairwise_combine(stacked, len(x)), stacked


@pytest.mark.parametrize("n", M.COMBINER_LENGTHS)
def test_combiner_equals_numpy_for_every_cut(n):
    x = sequence(n, n)
    mean = np.float32(np.add.reduce(x) / np.float32(n))
    want = {0: np.add.reduce(x), 1: np.add.reduce((x - mean) ** 2)}
    cuts_list = M.cut_lists(np.random.default_rng(n + 1), n)
    assert {len(c) for c in cuts_list} == {1, 2, 3, 8}
    for cuts in cuts_list:
        for mode in (0, 1):
            got, stacked = combine_cut(x, cuts, mode, mean)
            assert got.dtype == np.float32 and same_bits(got, want[mode]), (n, cuts, mode, got, want[mode])
        assert S.minmax_combine(stacked) == (float(x.min()), float(x.max())), (n, cuts)


def test_combiner_cuts_inside_every_kind_of_node():
    """one rank per element of a short sequence, and a cut at every position of a sequence with an irregular last piece"""
    x = sequence(300, 3)
    got, _ = combine_cut(x, [(i, i + 1) for i in range(300)], 0, 0.0)
    assert same_bits(got, np.add.reduce(x))
    x = sequence(8192 + 1500, 4)
    want = np.add.reduce(x)
    for c in list(range(8192 - 130, 8192 + 130)) + list(range(8192 + 600, 8192 + 900, 7)) + [len(x) - 1, len(x) - 3]:
        got, _ = combine_cut(x, [(0, c), (c, len(x))], 0, 0.0)
        assert same_bits(got, want), c


def test_combiner_refuses_ranges_that_do_not_tile():
    x = sequence(1000, 5)
    recs = np.stack([M.partial_record(x[0:400], 0, 1000, 0, 0.0), M.partial_record(x[500:], 500, 1000, 0, 0.0)])
    with pytest.raises(ValueError):
        S.pairwise_combine(recs, 1000)
    assert S.pairwise_combine(np.zeros((2, S.PW_REC_PIECES), np.float32), 0) == 0


def test_minmax_combine_nan_rules():
    """util.minmax: a NaN first element stays, any other NaN is ignored -- also when it is a later rank's first element"""
    x = np.array([3, np.nan, 1, np.nan, 7, 2], np.float32)
    recs = np.stack([M.partial_record(x[a:b], a, 6, 0, 0.0) for a, b in ((0, 3), (3, 6))])
    assert S.minmax_combine(recs) == (1.0, 7.0)
    x[0] = np.nan
    recs = np.stack([M.partial_record(x[a:b], a, 6, 0, 0.0) for a, b in ((0, 0), (0, 3), (3, 6))])
    assert all(np.isnan(v) for v in S.minmax_combine(recs))


# ---- detect_noise_level ----------------------------------------------------------------------------------------------------------
def sharded_noise(x, bounds):
    n = len(x)

    def work(r, comm):
        a, b = bounds[r]
        return S.ShardedPipeline(M.ModelEstimatorEngine(), comm).detect_noise_level(x[a:b], pos_base=a, n_total=n)
    got, err = M.run_ranks(len(bounds), work)
    assert not any(err), err
    return got


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [3, 4, 99, 199, 6400, 100_003])
def test_noise_level_equals_oracle(oracle, n, world):
    x = M.bursty_capture(n, n + world)
    want = oracle.detect_noise_level(oracle.get_magnitudes(x))
    got = sharded_noise(x, M.bounds_for(n, world))
    assert all(g == want for g in got), (got, want)
    if n > 100:
        assert want > 0


def test_noise_level_chunks_straddle_boundaries(oracle):
    """chunk 0 = [6336, 6400) and chunk 1 = [6272, 6336) are both cut by a shard boundary; a shard inside one chunk; an empty shard"""
    n = 6400
    x = M.bursty_capture(n, 9)[::-1].copy()                  # the quiet part at the end: the last chunks decide
    want = oracle.detect_noise_level(oracle.get_magnitudes(x))
    assert want > 0
    for bounds in ([(0, 6300), (6300, 6370), (6370, n)], [(0, 6300), (6300, 6300), (6300, 6310), (6310, 6399), (6399, n)]):
        assert all(g == want for g in sharded_noise(x, bounds)), bounds


def test_noise_level_uint16_nan_magnitudes(oracle):
    """65535^2 + 65535^2 wraps to a negative C int: its square root is NaN, which the chunk's mean and max carry"""
    n = 6400
    x = M.bursty_capture(n, 11, np.uint16)
    x[n - 40] = 65535                                      # in the last chunk
    mags = oracle.get_magnitudes(x)
    assert np.isnan(mags[n - 40]) and np.isnan(mags).sum() == 1
    want = oracle.detect_noise_level(mags)
    for world in (1, 2, 3, 8):
        assert all(g == want for g in sharded_noise(x, M.bounds_for(n, world))), world
    # the partials themselves: NaN in chunk 0 of the rank that holds the sample, 0.0 / 0.0 where a rank holds nothing of a chunk
    part = M.ModelEstimatorEngine().noise_partials(x[3200:], 3200, n, 64, 100).numpy()
    assert np.isnan(part[1, 0]) and np.isnan(part[0, 0]) and part[1, 1] > 0 and not part[:, 50:].any()


# ---- detect_center -----------------------------------------------------------------------------------------------------------------
def sharded_center(x, bounds, max_size=None):
    def work(r, comm):
        a, b = bounds[r]
        return S.ShardedPipeline(M.ModelEstimatorEngine(), comm).detect_center(x[a:b], max_size)
    got, err = M.run_ranks(len(bounds), work)
    assert not any(err), err
    return got


def assert_center(oracle, x, bounds, max_size=None, expect_none=False):
    want = oracle.detect_center(x, max_size)
    got = sharded_center(x, bounds, max_size)
    assert (want is None) == expect_none
    if want is None:
        assert all(g is None for g in got), got
    else:
        assert all(g is not None and np.float64(g) == np.float64(want) for g in got), (got, want, bounds)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [5_000, 20_000, 60_000])
def test_center_equals_oracle(oracle, n, world):
    x = M.two_level(n, n + world)
    rng = np.random.default_rng(world)
    e = [0] + sorted(int(c) for c in rng.integers(0, n + 1, world - 1)) + [n]
    assert_center(oracle, x, [(e[r], e[r + 1]) for r in range(world)])
    assert_center(oracle, x, M.bounds_for(n, world), max_size=n // 3)
    assert_center(oracle, x, M.bounds_for(n, world), max_size=10 * n)


def test_center_none_on_every_rank(oracle):
    n = 9_000
    bounds = M.bounds_for(n, 3)
    assert_center(oracle, np.full(n, -4.0, np.float32), bounds, expect_none=True)              # nothing kept
    assert_center(oracle, np.full(n, 0.25, np.float32), bounds, expect_none=True)              # variance 0
    assert_center(oracle, M.two_level(n, 1), bounds, max_size=0, expect_none=True)               # cut to nothing
    x = np.full(n, -4.0, np.float32)
    x[4000:4010] = 0.5                                                                          # ten kept samples on one rank
    want = oracle.detect_center(x)
    assert all(g == want if want is not None else g is None for g in sharded_center(x, bounds))


def test_center_ranks_that_keep_nothing_or_little(oracle):
    n = 30_000
    x = M.two_level(n, 21)
    x[10_000:20_000] = -4.0                                # rank 1 of 3 keeps nothing
    assert_center(oracle, x, [(0, 10_000), (10_000, 20_000), (20_000, n)])
    x[15_000:15_100] = M.two_level(100, 22, noise_runs=False)   # ... fewer than 128
    assert_center(oracle, x, [(0, 10_000), (10_000, 20_000), (20_000, n)])
    assert_center(oracle, M.two_level(n, 23, noise_runs=False), M.bounds_for(n, 8))               # nothing filtered


def test_center_refusals_before_any_collective():
    """a rank that is wrong on its own raises before it enters a collective: the others are released, nobody hangs"""
    x = M.two_level(4_000, 2)

    def work(r, comm):
        sp = S.ShardedPipeline(M.ModelEstimatorEngine(), comm)
        return sp.detect_center(x[2000 * r:2000 * (r + 1)].astype(np.float64 if r == 1 else np.float32))
    _, err = M.run_ranks(2, work, timeout=60)
    assert isinstance(err[1], ValueError) and err[0] is not None
    sp = S.ShardedPipeline(M.ModelEstimatorEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="max_size"):
        sp.detect_center(x, max_size=-1)
    with pytest.raises(ValueError, match="inside the capture"):
        sp.detect_noise_level(M.bursty_capture(100, 1), pos_base=50, n_total=120)


def test_auto_center_needs_psk():
    """ASK / FSK: the fused hot kernel needs the center before the demodulated signal exists -- refused before any collective"""
    from urh_amd.pipeline import DemodParams
    sp = S.ShardedPipeline(M.ModelEstimatorEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0))
    for mod in ("FSK", "ASK"):
        with pytest.raises(ValueError, match="auto_center"):
            sp.iq_to_bits(np.zeros((100, 2), np.float32), DemodParams(mod, 1, 0.1, 0.0, 1.0, 5, 100, 0.1, 8, True), auto_center=True)
