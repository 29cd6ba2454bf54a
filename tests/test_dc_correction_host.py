"""DC correction without a GPU: the facts about numpy's expression that the kernels rest on, pinned by assertion, and the numpy model of the
chunked float32 sum (tests/model_dc.py) against np.mean / x - mean on every input the GPU test uses (tests/dc_cases.py), bit for bit."""
import os

import numpy as np
import pytest

import dc_cases
import model_dc
from conftest import GOLDEN_DIR


def _seq_sum(col):
    """s = +0.0; s = fl32(s + x[i])"""
    return np.cumsum(np.concatenate([np.zeros(1, np.float32), col]), dtype=np.float32)[-1]


# ---- numpy's facts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 100_000])
def test_numpy_mean_of_a_column_is_the_sequential_float32_sum(n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 2)) + 0.3).astype(np.float32)
    mean = np.mean(x, axis=0)
    assert mean.dtype == np.float32
    pairwise_differs = 0
    for col in range(2):
        seq = _seq_sum(x[:, col])
        assert seq == np.cumsum(x, axis=0, dtype=np.float32)[-1, col]
        assert mean[col] == np.float32(np.float64(seq) / n)
        pairwise_differs += np.sum(np.ascontiguousarray(x[:, col])) != seq
    assert pairwise_differs, "the column sum is not numpy's pairwise sum"


def test_numpy_sum_starts_at_plus_zero():
    x = np.full((9, 2), -0.0, np.float32)
    mean = np.mean(x, axis=0)
    assert not np.signbit(mean).any()                       # +0.0 + -0.0 = +0.0
    assert np.signbit(x - mean).all()                       # -0.0 - +0.0 = -0.0


def test_numpy_divides_in_float64_by_the_exact_n():
    n = 2 ** 24 + 3                                         # not a float32
    assert float(np.float32(n)) != n
    x = np.empty((n, 2), np.float32)
    x[:, 0] = 0.75
    x[:, 1] = -0.375
    x[::7, 0] = 0.25
    mean = np.mean(x, axis=0)
    differs = 0
    for col in range(2):
        s = np.cumsum(x[:, col], dtype=np.float32)[-1]
        assert mean[col] == np.float32(np.float64(s) / np.float64(n))
        differs += mean[col] != s / np.float32(n)
    assert differs, "a float32 division would have given the same: the case proves nothing"


def test_numpy_integer_cast_truncates_and_wraps():
    assert np.array([227.9]).astype(np.int8)[0] == -29
    assert np.array([-1.5]).astype(np.uint16)[0] == 65535
    assert np.array([-40000.0]).astype(np.uint16)[0] == 25536
    for name, x in dc_cases.int_cases(2001).items():
        out, mean = dc_cases.numpy_dc(x)
        assert mean.dtype == np.float64
        m_mean, m_out = model_dc.dc_correct_int(x)
        assert dc_cases.same_bits(m_mean, mean) and dc_cases.same_bits(m_out, out), name
    u16 = dc_cases.int_cases(2001)["uint16_wrap"]
    out, mean = dc_cases.numpy_dc(u16)
    below = u16[:, 0] < mean[0]
    assert below.any() and (out[below, 0] > 32768).all()    # every sample below the mean wraps


# ---- the model of the chunked sum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc_cases.SIZES)
@pytest.mark.parametrize("name", sorted(dc_cases.F32_CASES))
def test_model_equals_numpy(name, n):
    x, want_out, want_mean = dc_cases.f32_case(name, n)
    mean, out, stats = model_dc.dc_correct_f32(x)
    assert dc_cases.same_bits(mean, want_mean), (mean, want_mean, stats)
    assert dc_cases.same_bits(out, want_out)
    n_chunks = -(-n // model_dc.CHUNK)
    assert stats["same"] + stats["moved"] + stats["redo"] == 2 * n_chunks
    if name in dc_cases.TRANSLATED_CASES:
        assert stats["redo"] <= dc_cases.redo_bound(n), stats
    if name == "zero_mean_spiked":
        assert stats["redo"] == 2 * (n_chunks - 1), stats
    if name in ("ties_even_k", "ties_odd_k", "odd_guess_ties"):
        assert stats["redo"] == 0 and stats["moved"] >= 2 * (n_chunks - 2), stats      # ties cost nothing: one path is an even distance away


@pytest.mark.parametrize("n", [1, 2, 7, 4095, 4096, 4097, 8192, 8193, 12289])
def test_model_sizes(n):
    x = dc_cases.generic(np.float32, n)
    want_out, want_mean = dc_cases.numpy_dc(x)
    mean, out, stats = model_dc.dc_correct_f32(x)
    assert dc_cases.same_bits(mean, want_mean) and dc_cases.same_bits(out, want_out)
    assert (stats["chunks"] == 0) == (n <= model_dc.DIRECT_MAX)


@pytest.mark.parametrize("off", [-3, -2, -1, 1, 2, 3, 1001, -100_000])
def test_model_is_exact_for_any_guess(off):
    """the guess only decides the cost: entries moved by `off` ulps, both parities, far enough to leave the margins"""
    n = 40_000
    x = dc_cases.generic(np.float32, n, seed=5)
    sums = np.add.reduceat(x.astype(np.float64), np.arange(0, n, model_dc.CHUNK), axis=0)
    guess = np.concatenate([np.zeros((1, 2)), np.cumsum(sums, axis=0)[:-1]]).astype(np.float32)
    moved = (guess.view(np.int32) + np.int32(off)).view(np.float32)
    moved[0] = guess[0]
    want_out, want_mean = dc_cases.numpy_dc(x)
    mean, out, _ = model_dc.dc_correct_f32(x, guess=moved)
    assert dc_cases.same_bits(mean, want_mean) and dc_cases.same_bits(out, want_out)


# ---- the fixtures recorded from the reference ---------------------------------------------------------------------------------------------
def test_fixtures_hold_the_reference_expression():
    d = os.path.join(GOLDEN_DIR, "dc")
    names = sorted(f for f in os.listdir(d) if f.endswith(".npz"))
    assert len({str(np.load(os.path.join(d, f))["iq"].dtype) for f in names}) >= 3
    for f in names:
        z = np.load(os.path.join(d, f), allow_pickle=False)
        iq = z["iq"]
        want, _ = dc_cases.numpy_dc(iq)
        assert dc_cases.same_bits(z["work"], want), f
        start, end = int(z["start"]), int(z["end"])
        part, _ = dc_cases.numpy_dc(iq[start:end])
        assert dc_cases.same_bits(z["range_iq"][start:end], part), f
        assert dc_cases.same_bits(z["range_iq"][:start], iq[:start]) and dc_cases.same_bits(z["range_iq"][end:], iq[end:]), f


# ---- the boundary, without a GPU ------------------------------------------------------------------------------------------------------------
def test_entry_points_and_argument_errors():
    from urh_amd import _lib
    from urh_amd.filter import Filter, FilterType
    lib = _lib.load()
    assert lib.urhgpu_dc_correct_dev(None, None, 4, _lib.DT_F32, None, None) == _lib.ERR_ARG
    assert lib.urhgpu_dc_correct(None, None, 4, _lib.DT_F32, None, None) == _lib.ERR_ARG
    assert lib.urhgpu_test_dc_stats(None, None) == _lib.ERR_ARG
    assert lib.urhgpu_test_dc_host_syncs() >= 0
    assert {t.name for t in FilterType} == {"moving_average", "dc_correction", "custom"}
    assert Filter([1.0]).filter_type == FilterType.custom


def test_sharded_passes_refuse_dc_correction():
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    sp = ShardedPipeline(None, ThreadComm(ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="sharded"):
        sp.iq_to_bits(None, DemodParams(), dc_correction=True)


def test_no_cpu_fallback():
    import torch
    from urh_amd import _lib
    from urh_amd.filter import Filter, FilterType
    flt = Filter([], FilterType.dc_correction)
    if torch.cuda.is_available():
        assert dc_cases.same_bits(flt.work(np.ones((8, 2), np.float32)), np.zeros((8, 2), np.float32))
        return
    with pytest.raises(_lib.UrhGpuError):
        flt.work(np.zeros((8, 2), np.float32))
