"""The live sniffer on the GPU: GpuSniffEngine (urhgpu_chunk_power_stats_dev + DevicePipeline) must reproduce the reference's recorded live
runs (tests/golden/sniffer/) exactly, with the chunks fed as numpy arrays and as device tensors, and the per-chunk kernel must match
numpy bit for bit.  Reads committed fixtures only."""
import ctypes as C

import numpy as np
import pytest

import model_sniffer as ms
from test_sniffer_host import EXPECTED_CASES

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.int8, np.uint8, np.int16, np.uint16]
# row counts around the pairwise geometry (2n floats: leaves of 128, pieces of 8192) and the 16-byte accesses
ROW_COUNTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 100003, (1 << 20) + 5]


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def _tdtype(torch, dtype):
    return {np.float32: torch.float32, np.int8: torch.int8, np.uint8: torch.uint8, np.int16: torch.int16, np.uint16: torch.uint16}[dtype]


def _random_rows(rng, n, dtype):
    if dtype == np.float32:
        return (rng.standard_normal((n, 2)) * rng.choice([1e-3, 1.0, 30.0])).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(dtype)


def _stats(pipe, src, code, n, dst_ptr, n_store):
    from urh_amd import _lib
    s, m = C.c_double(0.0), C.c_double(0.0)
    pipe.ctx.set_stream(pipe.torch.cuda.current_stream(pipe.device).cuda_stream)
    _lib.check(_lib.load().urhgpu_chunk_power_stats_dev(pipe.ctx.handle, C.c_void_p(src.data_ptr()), code, n, C.c_void_p(dst_ptr), n_store,
                                                        C.byref(s), C.byref(m)))
    return s.value, m.value


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_stats_match_numpy(pipe, dtype):
    """np.mean(c ** 2.0) and np.max(c ** 2.0) bit for bit, the chunk a slice at an odd row offset of a larger buffer; the destination rows
    equal the source, the rows beyond the stored (trimmed) length and in front of the destination are untouched"""
    import torch
    from urh_amd.signal_functions import dtype_code
    rng = np.random.default_rng(5)
    code, ft = dtype_code(np.dtype(dtype)), (np.float32 if dtype == np.float32 else np.float64)
    for k, n in enumerate(ROW_COUNTS):
        off_src, off_dst = 1 + 2 * (k % 3), 3 + (k % 4)                 # odd source offsets; destination offsets of either parity
        host = _random_rows(rng, n + off_src + 2, dtype)
        big = torch.from_numpy(host).to(pipe.device)
        c = host[off_src:off_src + n]
        n_store = n if k % 2 == 0 else max(n - 1 - k % 3, 0)            # every other case trims the append
        guard = _random_rows(rng, n + off_dst + 5, dtype)
        dst = torch.from_numpy(guard).to(pipe.device)
        got_sum, got_max = _stats(pipe, big[off_src:off_src + n], code, n, dst[off_dst:].data_ptr(), n_store)
        with np.errstate(all="ignore"):
            want_mean, want_max = np.mean(c ** 2.0), np.max(c ** 2.0)
        assert want_mean.dtype == ft and want_max.dtype == ft
        got_mean = ft(got_sum) / ft(2 * n)
        print(f"{np.dtype(dtype).name} n={n}: mean {got_mean!r} / {want_mean!r}  max {ft(got_max)!r} / {want_max!r}")
        assert _same_bits(got_mean, want_mean), (n, got_mean, want_mean)
        assert _same_bits(ft(got_max), want_max), (n, got_max, want_max)
        out = dst.cpu().numpy()
        want_out = guard.copy()
        want_out[off_dst:off_dst + n_store] = c[:n_store]
        assert out.tobytes() == want_out.tobytes(), n
        # statistics only (the chunk already lies in the buffer): the same numbers, nothing written
        again = _stats(pipe, big[off_src:off_src + n], code, n, None, 0)
        assert _same_bits(np.float64(again[0]), np.float64(got_sum)) and _same_bits(np.float64(again[1]), np.float64(got_max))
        assert big.cpu().numpy().tobytes() == host.tobytes()


def test_chunk_stats_nan_inf(pipe):
    import torch
    from urh_amd import _lib
    rng = np.random.default_rng(6)
    for n, where, val in ((100, 17, np.nan), (5000, 4999, np.nan), (5000, 0, np.inf), (3, 2, -np.inf), (20000, 12345, np.nan)):
        c = rng.standard_normal((n, 2)).astype(np.float32)
        c[where, 1] = val
        s, m = _stats(pipe, torch.from_numpy(c).to(pipe.device), _lib.DT_F32, n, None, 0)
        with np.errstate(all="ignore"):
            want_mean, want_max = np.mean(c ** 2.0), np.max(c ** 2.0)
        assert _same_bits(np.float32(s) / np.float32(2 * n), want_mean) and _same_bits(np.float32(m), want_max)


def test_chunk_stats_argument_errors(pipe):
    import torch
    from urh_amd import _lib
    lib, h = _lib.load(), pipe.ctx.handle
    s, m = C.c_double(), C.c_double()
    x = torch.zeros((16, 2), dtype=torch.float32, device=pipe.device)
    p = C.c_void_p(x.data_ptr())
    assert lib.urhgpu_chunk_power_stats_dev(h, p, _lib.DT_F32, 0, None, 0, C.byref(s), C.byref(m)) == _lib.ERR_ARG
    assert lib.urhgpu_chunk_power_stats_dev(h, p, 9, 16, None, 0, C.byref(s), C.byref(m)) == _lib.ERR_DTYPE
    assert lib.urhgpu_chunk_power_stats_dev(h, p, _lib.DT_F32, 16, None, 17, C.byref(s), C.byref(m)) == _lib.ERR_ARG
    assert lib.urhgpu_chunk_power_stats_dev(h, p, _lib.DT_F32, 8, C.c_void_p(x[4:].data_ptr()), 8, C.byref(s), C.byref(m)) == _lib.ERR_ARG   # overlap


@pytest.mark.parametrize("feed_as", ["numpy", "device"])
@pytest.mark.parametrize("name", EXPECTED_CASES)
def test_gpu_sniffer_equals_reference(pipe, name, feed_as):
    import torch
    from urh_amd.sniffer import GpuSniffEngine
    g = ms.load_case(name)
    engine = GpuSniffEngine(pipe, g["iq"].dtype, g["buffer_samples"])
    sniffer = ms.make_sniffer(g, engine, pipe)
    if feed_as == "numpy":
        chunks = ms.chunks_of(g)
    else:
        dev = torch.from_numpy(g["iq"]).to(pipe.device)
        chunks = (dev[a:b] for a, b in zip(np.cumsum(g["chunk_lens"]) - g["chunk_lens"], np.cumsum(g["chunk_lens"])))
    before = engine.launches()
    ms.check_against_fixture(g, sniffer, chunks)
    # a fed chunk issues a fixed number of launches, independent of its length (counter: urhgpu_chunk_stats_launches)
    assert engine.launches() - before == 2 * int((g["chunk_lens"] > 0).sum())


def test_launches_per_chunk_do_not_depend_on_length(pipe):
    import torch
    from urh_amd.sniffer import GpuSniffEngine
    engine = GpuSniffEngine(pipe, np.float32, 3_000_000)
    for n in (1, 100, 8192, 200_000, 2_000_000):
        for chunk in (np.ones((n, 2), np.float32), torch.ones((n, 2), dtype=torch.float32, device=pipe.device)):
            before = engine.launches()
            engine.stats_append(chunk, 5)
            assert engine.launches() - before == 2, n


def test_default_engine_and_default_buffer(pipe):
    """LiveSniffer without an engine builds the GPU engine with the reference's 12.5 M row buffer"""
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import GpuSniffEngine, LiveSniffer
    sn = LiveSniffer(pipe, DemodParams("FSK", 1, 0.1, 0.0), dtype=np.int8)
    assert isinstance(sn.engine, GpuSniffEngine) and sn.engine.buffer.shape == (12_500_000, 2) and sn.buffer_len == 12_500_000
    assert sn.feed(np.full((1000, 2), 50, np.int8)) == [] and sn.index == 1000 and sn.pause_length == 0
    assert sn.engine.buffer[:1000].cpu().numpy().tobytes() == np.full((1000, 2), 50, np.int8).tobytes()
