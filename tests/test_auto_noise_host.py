"""The automatic noise threshold, host side (no GPU): tests/model_noise.py -- the numpy model of k_noise_decide with every scalar type
spelled out -- against the oracle's detect_noise_level and against the real reference's thresholds recorded in
tests/golden/auto_noise.json; the flag arithmetic of include/urhgpu.h (urhgpu_noise_result); the library's host-side pieces."""
import math

import numpy as np
import pytest

import model_noise as mn
import noise_cases as nc


def oracle_value(oracle, iq):
    return oracle.detect_noise_level(oracle.get_magnitudes(iq))


@pytest.mark.parametrize("dtype", nc.DTYPES5, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", nc.HOST_SIZES)
def test_model_equals_the_oracle(oracle, n, dtype):
    """seeded captures at the sizes where the chunk geometry changes, five sample types"""
    iq = nc.capture(7 + n, n, dtype=dtype)
    want = oracle_value(oracle, iq)
    got, flag = mn.detect(oracle.get_magnitudes(iq), dtype)
    assert got == want and flag == 1, (n, np.dtype(dtype).name, got, want, flag)
    assert mn.chunk_geometry(n)[1] <= 199


def test_model_on_degenerate_captures(oracle):
    n = 60000
    zero = np.zeros((n, 2), np.float32)
    assert mn.detect(oracle.get_magnitudes(zero), np.float32) == (0.0, 1) and oracle_value(oracle, zero) == 0
    const = nc.constant_envelope(n)
    assert oracle_value(oracle, const) == 0                                # ratio of the means > 0.9
    noise, flag, cand, lo, hi = mn.decide(*mn.chunk_stats(oracle.get_magnitudes(const)), mn.max_magnitude(np.float32))
    assert (noise, flag, cand) == (0.0, 1, 0) and lo / hi > 0.9
    # quiet chunks whose means tie exactly on 1.1f * min: magnitudes 1.0 in the quietest chunk and fl32(1.1f * 1.0f) in the next two -- both
    # candidates (<=), with the larger maximum; a loud rest
    chunk = n // 100
    mag = np.full(n, 40.0)
    tie = float(np.float32(1.1) * np.float32(1.0))
    mag[n - chunk:] = 1.0
    mag[n - 3 * chunk:n - chunk] = tie
    mag[n - 2 * chunk] = tie                                               # (the chunk's maximum is its constant value)
    noise, flag, cand, _, _ = mn.decide(*mn.chunk_stats(mag), mn.max_magnitude(np.int16))
    assert cand == 3 and flag == 1
    assert noise == oracle.detect_noise_level(mag) == math.ceil(tie * 10000) / 10000


def test_model_and_oracle_reproduce_the_reference_fixture(oracle):
    """every threshold the REAL reference computed (tests/golden/make_auto_noise_golden.py), bit for bit"""
    gold = nc.load_golden()
    assert set(gold) == set(nc.pass_cases())
    for name, g in gold.items():
        assert g["recipe"] == nc.pass_cases()[name], name
        iq = nc.case_capture(g["recipe"])
        want = float.fromhex(g["threshold"])
        mag = oracle.get_magnitudes(iq)
        assert oracle.detect_noise_level(mag) == want, name
        noise, flag = mn.detect(mag, iq.dtype)
        assert noise == want and flag == (2 if g["gates_all"] else 1), (name, noise, want, flag)
    assert gold["gates-all"]["gates_all"] and gold["gates-all"]["bits"] == []
    assert sum(g["gates_all"] for g in gold.values()) == 1


@pytest.mark.parametrize("dtype", nc.DTYPES5, ids=lambda d: np.dtype(d).name)
def test_flag_2_is_the_gate_of_quad_demod(dtype):
    """noise < Signal.max_magnitude as a comparison of doubles (Signal.py:474-484): a maximum one step below the bound that still rounds
    up to a value below it is flag 1; at the bound and beyond: flag 2"""
    mm = mn.max_magnitude(dtype)
    from urh_amd import _lib, signal_functions as sf
    assert _lib.load().urhgpu_noise_max_magnitude(sf.dtype_code(dtype)) == mm
    below = math.floor(mm * 10000 - 1) / 10000
    for value, flag in ((below, 1), (mm, 2), (mm * 2, 2)):
        sums, maxs = np.array([1.0, 50.0 * mm]), np.array([value, 100.0 * mm])        # one quiet chunk of one sample
        noise, got, cand, _, _ = mn.decide(sums, maxs, 1, mm)
        assert cand == 1 and got == flag and noise == math.ceil(value * 10000) / 10000, (value, noise, got)
        f32, sq = mn.block_values(noise, got, 0.25, in_pass=True)
        assert (f32 == np.float32(noise)) == (flag == 1) and sq == np.float32(f32 * f32)
        assert mn.block_values(noise, got, 0.25, in_pass=False)[0] == np.float32(noise)


def test_flag_0_where_math_ceil_raises():
    """NaN and infinite statistics: the reference's math.ceil raises ValueError / OverflowError -- unless a NaN MEAN keeps every chunk
    from comparing, where it returns 0"""
    from urh_amd.pipeline import raise_noise_error
    mm = mn.max_magnitude(np.float32)
    noise, flag, _, _, _ = mn.decide(np.array([1.0, 50.0]), np.array([math.nan, 60.0]), 1, mm)       # a candidate whose maximum is a NaN
    assert flag == 0 and math.isnan(noise)
    with pytest.raises(ValueError):
        raise_noise_error(noise)
    noise, flag, _, _, _ = mn.decide(np.array([math.inf, math.inf]), np.array([math.inf, math.inf]), 1, mm)
    assert flag == 0 and noise == math.inf
    with pytest.raises(OverflowError):
        raise_noise_error(noise)
    # one infinite chunk among finite ones is no candidate: the value is that of the quiet chunk
    assert mn.decide(np.array([1.0, math.inf]), np.array([1.0, math.inf]), 1, mm)[:2] == (1.0, 1)
    # a NaN mean anywhere: np.min is NaN, nothing compares, np.max([]) -> ValueError -> detect_noise_level returns 0
    for sums in ([math.nan, 50.0], [1.0, math.nan, 50.0]):
        assert mn.decide(np.array(sums), np.array(sums), 1, mm)[:2] == (0.0, 1)


def test_the_oracle_on_non_finite_captures(oracle):
    """what the flag-0 GPU tests rely on: a NaN sample makes its chunk's mean a NaN -- detect_noise_level returns 0 --, an all-infinite
    capture reaches math.ceil(inf)"""
    iq = np.array(nc.capture(11, 60000))
    iq[100, 0] = np.nan
    assert oracle_value(oracle, iq) == 0 and mn.detect(oracle.get_magnitudes(iq), np.float32) == (0.0, 1)
    inf = np.full((60000, 2), np.inf, np.float32)
    with pytest.raises(OverflowError):
        oracle_value(oracle, inf)
    assert mn.detect(oracle.get_magnitudes(inf), np.float32) == (math.inf, 0)


def test_result_block_layout():
    import ctypes as C
    from urh_amd import _lib
    assert C.sizeof(_lib.NoiseResult) == 64
    assert [(f, getattr(_lib.NoiseResult, f).offset) for f, _ in _lib.NoiseResult._fields_] == \
        [("noise", 0), ("noise_f32", 8), ("noise_sqrd", 12), ("flag", 16), ("chunk", 24), ("n_chunks", 32), ("n_candidates", 40), ("min_mean", 48),
         ("max_mean", 56)]


def test_argument_errors_without_gpu():
    import ctypes as C
    from urh_amd import _lib
    lib = _lib.load()
    null = C.c_void_p(None)
    assert lib.urhgpu_detect_noise_level_dev(null, null, 4, 10, null) == _lib.ERR_ARG
    assert lib.urhgpu_iq_to_bits_auto_dev(null, null, 10, None, 1, 0, -1, None, null, null, null, null, 0) == _lib.ERR_ARG
    assert lib.urhgpu_stream_set_auto_noise(null, 1) == _lib.ERR_ARG
    assert lib.urhgpu_stream_noise(null, 0, None, None) == _lib.ERR_ARG
    assert lib.urhgpu_test_noise_host_syncs() >= 0
    assert lib.urhgpu_noise_max_magnitude(99) == 0.0
