"""The filter kernels (urh_amd/csrc/filters.hip: k_fir, k_fir_fast, the statistics epilogue, k_iir_*) against the oracle on the inputs of
tests/filter_cases.py, bit for bit (NaN equal to NaN); the reference itself is seen through tests/golden/filter/edges.npz.  The one
tolerance is the chunk SUMS of the fused statistics, which the kernel adds in its own order (filter_cases.sum_bound).
tests/test_filters_host.py pins the oracle on the same inputs.  Run on the GPU box:  python -m pytest tests/test_filters_gpu.py -m gpu
"""
import ctypes as C
import math

import numpy as np
import pytest

import filter_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sf():
    from urh_amd import signal_functions
    return signal_functions


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline()


@pytest.fixture(scope="module")
def golden():
    return F.load_golden()


@pytest.fixture(scope="module")
def a_ref(oracle):
    """{name: (samples, taps, the oracle's result)} of family A, computed once"""
    return {name: (x, h, oracle.fir_filter(x, h)) for name, x, h in F.a_cases()}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None


def fir_dev(ctx, x, h, halo=None):
    """urhgpu_fir_filter_dev on the current torch stream -> host array"""
    import torch
    from urh_amd import _lib
    dx, dh, dl = _dev(x), _dev(h), _dev(halo)
    out = torch.empty_like(dx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().urhgpu_fir_filter_dev(ctx.handle, _ptr(dx), len(x), _ptr(dh), len(h), _ptr(dl), _ptr(out)))
    return out.cpu().numpy()


def fir_stats_dev(ctx, x, h, halo, chunk, n_chunks):
    """urhgpu_fir_filter_stats_dev -> (filtered, sums, maxima) on the host"""
    import torch
    from urh_amd import _lib
    dx, dh, dl = _dev(x), _dev(h), _dev(halo)
    out = torch.empty_like(dx)
    sums = torch.full((n_chunks,), -1.0, dtype=torch.float64, device="cuda")
    maxs = torch.full((n_chunks,), -1.0, dtype=torch.float64, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().urhgpu_fir_filter_stats_dev(ctx.handle, _ptr(dx), len(x), _ptr(dh), len(h), _ptr(dl), _ptr(out), chunk, n_chunks,
                                                       _ptr(sums), _ptr(maxs)))
    return out.cpu().numpy(), sums.cpu().numpy(), maxs.cpu().numpy()


# ---- A: tap counts -------------------------------------------------------------------------------------------------------------------------
A_NAMES = ["preset_Very_Narrow", "preset_Narrow", "preset_Medium", "preset_Wide", "preset_Very_Wide", "preset_Very_Narrow_n1000",
           "random_2768", "random_2769", "random_5232", "random_5233", "random_7950"]


@pytest.mark.parametrize("name", A_NAMES)
def test_fir_tap_counts_equal_oracle(sf, a_ref, golden, name):
    """the reference's own preset filters (11 ... 4001 taps) and the tap counts either side of each LDS threshold of launch_fir"""
    assert sorted(a_ref) == sorted(A_NAMES)
    x, h, want = a_ref[name]
    got = sf.fir_filter(x, h)
    assert F.same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if name in golden["fir"]:
        assert F.same_bits(got, golden["fir"][name][2])


def test_fir_tap_limit_is_where_the_formula_puts_it(sf, a_ref, oracle):
    """7950 taps are accepted, 7951 refused with ERR_UNSUPPORTED, and the context filters exactly right after the refusal"""
    from urh_amd import _lib
    x, h, want = a_ref[f"random_{F.M_MAX}"]
    assert len(h) == 7950 and F.same_bits(sf.fir_filter(x, h), want)
    with pytest.raises(_lib.UrhGpuError) as e:
        sf.fir_filter(x, np.concatenate([h, h[:1]]))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    assert F.same_bits(sf.fir_filter(x, h[:5]), oracle.fir_filter(x, h[:5]))


@pytest.mark.parametrize("case", F.a_halo_cases(), ids=lambda c: c[0])
def test_fir_long_filter_with_left_halo_equals_one_pass(pipe, oracle, case):
    """401 and 4001 taps: a shard cut at an index that is no multiple of 8, filtered with the m - 1 samples before it as halo"""
    name, x, h, cut = case
    want = oracle.fir_filter(x, h)[cut:]
    got = fir_dev(pipe.ctx, x[cut:], h, x[cut - (len(h) - 1):cut])
    assert F.same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_fir_work_area_grows_and_waits_across_streams(oracle):
    """one context: a small filter, the largest one on another stream, a small one again on the first, queued without waiting for the
    device in between -- the work area grows for the second call and the third waits for the second's event"""
    import torch
    from urh_amd import _lib
    ctx = _lib.Context(0)
    lib = _lib.load()
    seq = F.a_sequence()
    dev = [(_dev(x), _dev(h), torch.empty(len(x), dtype=torch.complex64, device="cuda")) for x, h in seq]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for i, (dx, dh, out) in enumerate(dev):
        stream = side if i == 1 else torch.cuda.current_stream()
        ctx.set_stream(stream.cuda_stream)
        _lib.check(lib.urhgpu_fir_filter_dev(ctx.handle, _ptr(dx), dx.shape[0], _ptr(dh), dh.shape[0], None, _ptr(out)))
    torch.cuda.synchronize()
    for i, ((x, h), (_, _, out)) in enumerate(zip(seq, dev)):
        assert F.same_bits(out.cpu().numpy(), oracle.fir_filter(x, h)), i


# ---- B: the checked kernel behind the fast one ---------------------------------------------------------------------------------------------
def test_fir_every_tile_handed_back_more_than_the_grid(sf, oracle):
    """an infinite tap sends all 1026 tiles to the checked kernel, which works the list off with 1024 workgroups: a second trip"""
    x, h = F.b_every_tile()
    with np.errstate(all="ignore"):
        want = oracle.fir_filter(x, h)
    got = sf.fir_filter(x, h)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))
    assert same.all(), (int((~same).sum()), np.nonzero(~same)[0][:4] // 2 // F.TILE)


def test_fir_tile0_handed_back_with_halo(pipe, oracle):
    """the halo ends in nan, inf, 1e30: tile 0 goes to the checked kernel, which must read the halo as the fast one does"""
    halo, x, h = F.b_halo_tile0()
    with np.errstate(all="ignore"):
        want = oracle.fir_filter(np.concatenate([halo, x]), h)[len(halo):]
    assert F.same_bits(fir_dev(pipe.ctx, x, h, halo), want)


@pytest.mark.parametrize("at", [False, True], ids=["below", "at"])
def test_fir_safe_threshold(sf, oracle, golden, at):
    """largest component one float below 2^60 (fast kernel) and exactly 2^60 (handed back): the sums overflow to +inf from output 256 on"""
    x, h = F.b_threshold(at)
    with np.errstate(all="ignore"):
        want = oracle.fir_filter(x, h)
    got = sf.fir_filter(x, h)
    assert F.same_bits(got, want) and F.same_bits(got, golden["fir"]["threshold_at" if at else "threshold_below"][2])


# ---- C: fused statistics, chunk by chunk ---------------------------------------------------------------------------------------------------
def _outcome(f, *args):
    try:
        return f(*args)
    except (ValueError, OverflowError) as e:               # math.ceil of a NaN / an infinite maximum, as in the reference
        return type(e).__name__


@pytest.mark.parametrize("variant", F.C_VARIANTS)
@pytest.mark.parametrize("with_halo", [False, True], ids=["nohalo", "halo"])
@pytest.mark.parametrize("geometry", F.C_GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}")
def test_fir_fused_statistics_chunk_by_chunk(pipe, oracle, geometry, with_halo, variant):
    """urhgpu_fir_filter_stats_dev with a free chunk size on 11 017 samples.  Maxima: np.max of the chunk exactly, NaN where it holds one.
    Sums: within chunk * 2^-52 * fsum(chunk) of math.fsum (filter_cases.sum_bound); a chunk with a NaN gives NaN; a chunk whose exact sum
    is infinite (the 3e24 sample: its magnitudes overflow float32) gives +inf.  Filtered samples: those of urhgpu_fir_filter_dev."""
    from urh_amd.estimators import noise_level_from_chunk_stats
    chunk, n_chunks = geometry
    halo, x, h = F.c_case(chunk, n_chunks, variant, with_halo)
    with np.errstate(all="ignore"):
        want_y, chunks = F.c_reference(oracle, halo, x, h, chunk, n_chunks)
    plain = fir_dev(pipe.ctx, x, h, halo)
    got_y, sums, maxs = fir_stats_dev(pipe.ctx, x, h, halo, chunk, n_chunks)
    assert F.same_bits(plain, want_y)
    assert np.array_equal(got_y.view(np.uint32), plain.view(np.uint32))
    with np.errstate(all="ignore"):
        want_max = np.array([np.max(c) for c in chunks])
    print("maxima", maxs, want_max)
    assert np.array_equal(maxs, want_max, equal_nan=True)
    want_sums = []
    for k, c in enumerate(chunks):
        if np.isnan(c).any():
            want_sums.append(float("nan"))
            assert math.isnan(sums[k]), (k, sums[k])
            continue
        exact = math.fsum(c)
        want_sums.append(exact)
        print("chunk", k, "sum", sums[k], "exact", exact, "bound", F.sum_bound(c))
        if math.isinf(exact):
            assert sums[k] == exact, (k, sums[k])
        else:
            assert abs(sums[k] - exact) <= F.sum_bound(c), (k, sums[k], exact, F.sum_bound(c))
    with np.errstate(all="ignore"):
        assert _outcome(noise_level_from_chunk_stats, sums, maxs, chunk) == _outcome(noise_level_from_chunk_stats, want_sums, want_max, chunk)


# ---- D: IIR --------------------------------------------------------------------------------------------------------------------------------
D_CASES = F.d_cases()


@pytest.mark.parametrize("case", D_CASES, ids=lambda c: c[0])
def test_iir_equals_oracle_and_reference(sf, oracle, golden, case):
    """sizes around max(M, N + 1), M = 0, non-finite / signed-zero / denormal samples and coefficients, feedback that overflows: the
    complex128 product keeps a sample with two infinite parts infinite (C99 Annex G), as the reference's does"""
    name, a, b, x = case
    with np.errstate(all="ignore"):
        want = oracle.iir_filter(a, b, x)
    got = sf.iir_filter(a, b, x)
    bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)))))[0]
    assert got.shape == want.shape and len(bad) == 0, (len(bad), bad[:4] // 2, got[bad[:4] // 2], want[bad[:4] // 2])
    assert F.same_bits(got, golden["iir"][name][3])


# ---- E: empty taps -------------------------------------------------------------------------------------------------------------------------
def test_fir_empty_taps_as_the_reference(sf, golden):
    """the host functions return what the reference returns: n - 1 zeros for no taps, ValueError for no taps and no samples, an empty array
    for no samples"""
    from urh_amd.filter import Filter
    for name, (x, h, kind, y) in golden["empty"].items():
        for fir in (sf.fir_filter, lambda xs, taps: Filter(taps).work(xs)):
            got_kind, got = F.fir_outcome(fir, x, h)
            assert got_kind == kind, name
            if kind == "array":
                assert got.dtype == np.complex64 and got.shape == y.shape and F.same_bits(got, y), name


def test_fir_empty_taps_c_abi_and_device_routes_keep_the_length(pipe):
    """urhgpu_fir_filter writes n zeros for m = 0, and filter.fir_filter_dev returns the capture's shape"""
    import torch
    from urh_amd import _lib
    from urh_amd.filter import fir_filter_dev
    x = F.e_cases()[0][1]
    out = np.ones(len(x), dtype=np.complex64)
    _lib.check(_lib.load().urhgpu_fir_filter(_lib.default_context().handle, C.c_void_p(x.ctypes.data), len(x), None, 0, C.c_void_p(out.ctypes.data)))
    assert not out.view(np.uint32).any()
    iq = torch.from_numpy(x.view(np.float32).reshape(-1, 2).copy()).cuda()
    y = fir_filter_dev(pipe, iq, np.zeros(0, np.complex64))
    assert tuple(y.shape) == (len(x), 2) and not y.cpu().numpy().view(np.uint32).any()
