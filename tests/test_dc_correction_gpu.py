"""DC correction on the GPU (urhgpu_dc_correct_dev and everything built on it) against numpy's own expression and the fixtures recorded
from the reference (tests/golden/dc/, tests/golden/make_dc_golden.py) -- never against the code under test.  The inputs and their numpy
results come from tests/dc_cases.py, where the host model is held against the same."""
import ctypes as C
import os

import numpy as np
import pytest

import dc_cases
from conftest import GOLDEN_DIR, synth_fsk
from dc_cases import numpy_dc, same_bits

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.float32]
SIZES = [1, 2, 7, 4095, 4096, 4097, 8193, 100_003]


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def dev(pipe, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(pipe.device)


def dc_stats(pipe):
    from urh_amd import _lib
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load().urhgpu_test_dc_stats(pipe.ctx.handle, out))
    return {"chunks": int(out[0]), "derived": int(out[1]), "redo": int(out[2]), "same": int(out[3])}


def host_syncs():
    from urh_amd import _lib
    return int(_lib.load().urhgpu_test_dc_host_syncs())


# ---- 1. the entry points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_sizes_and_forms(pipe, dtype, n):
    """out of place (the input untouched), in place, from a slice that starts on an odd sample (no 16-byte alignment), and the host form"""
    from urh_amd.filter import dc_correct, dc_correct_dev
    x = dc_cases.generic(dtype, n + 3)
    for off in (0, 3):
        part = x[off:off + n]
        want, want_mean = numpy_dc(part)
        big = dev(pipe, x)
        d_in = big[off:off + n]
        out, mean = dc_correct_dev(pipe, d_in, want_mean=True)
        assert same_bits(out.cpu().numpy(), want), (off, "out of place")
        assert same_bits(mean.cpu().numpy(), want_mean), (off, mean.cpu().numpy(), want_mean)
        assert same_bits(big.cpu().numpy(), x), "the input was modified"
        dc_correct_dev(pipe, d_in, out=d_in)
        after = big.cpu().numpy()
        assert same_bits(after[off:off + n], want), (off, "in place")
        assert same_bits(after[:off], x[:off]) and same_bits(after[off + n:], x[off + n:]), "rows outside the range were written"
    h_out, h_mean = dc_correct(x[:n], pipe.ctx, want_mean=True)
    want, want_mean = numpy_dc(x[:n])
    assert same_bits(h_out, want) and same_bits(h_mean, want_mean)


def test_empty_and_rejected(pipe):
    import torch
    from urh_amd import _lib
    from urh_amd.filter import dc_correct_dev
    lib, h = _lib.load(), pipe.ctx.handle
    assert lib.urhgpu_dc_correct_dev(h, None, 0, _lib.DT_F32, None, None) == _lib.OK
    t = torch.zeros((16, 2), dtype=torch.float32, device=pipe.device)
    assert lib.urhgpu_dc_correct_dev(h, C.c_void_p(t.data_ptr()), 8, 7, C.c_void_p(t.data_ptr()), None) == _lib.ERR_DTYPE
    assert lib.urhgpu_dc_correct_dev(h, C.c_void_p(t.data_ptr()), 8, _lib.DT_F32, C.c_void_p(t.data_ptr() + 8), None) == _lib.ERR_ARG   # overlap
    assert lib.urhgpu_dc_correct_dev(h, C.c_void_p(t.data_ptr() + 4), 4, _lib.DT_F32, C.c_void_p(t.data_ptr() + 4), None) == _lib.ERR_ARG   # half a sample
    with pytest.raises(ValueError):
        dc_correct_dev(pipe, torch.zeros((4, 2), dtype=torch.float64, device=pipe.device))


@pytest.mark.parametrize("n", dc_cases.SIZES)
@pytest.mark.parametrize("name", sorted(dc_cases.F32_CASES))
def test_float32_cases(pipe, name, n):
    from urh_amd.filter import dc_correct_dev
    x, want, want_mean = dc_cases.f32_case(name, n)
    out, mean = dc_correct_dev(pipe, dev(pipe, x), want_mean=True)
    got_mean = mean.cpu().numpy()
    st = dc_stats(pipe)
    print(name, n, "mean", got_mean, "numpy", want_mean, st)
    assert same_bits(got_mean, want_mean), (got_mean, want_mean, st)
    assert same_bits(out.cpu().numpy(), want)
    n_chunks = -(-n // dc_cases.CHUNK)
    assert st["chunks"] == n_chunks and st["derived"] + st["redo"] == 2 * n_chunks
    if name in dc_cases.TRANSLATED_CASES:
        # translation does the work: what is re-evaluated stays within what the binade edges on the sum's way can spoil
        assert st["redo"] <= dc_cases.redo_bound(n) and st["derived"] - st["same"] > st["redo"], st
    if name == "zero_mean_spiked":
        assert st["redo"] == 2 * (n_chunks - 1), st                  # every chunk behind the first (which is entered at +0.0, as guessed)
    if name == "neg_zero":
        assert np.signbit(out.cpu().numpy()).all() and not np.signbit(got_mean).any()


def test_float32_division_by_an_n_that_is_no_float32(pipe):
    """N = 2^24 + 3: numpy divides the float32 sum in float64 by the exact N (tests/test_dc_correction_host.py pins that a float32 division
    differs on this input)"""
    from urh_amd.filter import dc_correct_dev
    n = 2 ** 24 + 3
    x = np.empty((n, 2), np.float32)
    x[:, 0] = 0.75
    x[:, 1] = -0.375
    x[::7, 0] = 0.25
    want, want_mean = numpy_dc(x)
    d = dev(pipe, x)
    _, mean = dc_correct_dev(pipe, d, out=d, want_mean=True)
    assert same_bits(mean.cpu().numpy(), want_mean), (mean.cpu().numpy(), want_mean, dc_stats(pipe))
    assert same_bits(d.cpu().numpy(), want)


@pytest.mark.parametrize("name", ["int8_alternating", "uint8_around_128", "uint16_wrap", "int16_extremes"])
def test_integer_cases(pipe, name):
    from urh_amd.filter import dc_correct_dev
    x = dc_cases.int_cases()[name]
    want, want_mean = numpy_dc(x)
    out, mean = dc_correct_dev(pipe, dev(pipe, x), want_mean=True)
    assert same_bits(mean.cpu().numpy(), want_mean), (mean.cpu().numpy(), want_mean)
    assert same_bits(out.cpu().numpy(), want)
    if name == "uint16_wrap":
        below = x[:, 0] < want_mean[0]
        assert below.any() and (want[below, 0] > 32768).all()         # the case does wrap


# ---- 2. Filter and Signal.filter_range ----------------------------------------------------------------------------------------------------
def fixtures():
    d = os.path.join(GOLDEN_DIR, "dc")
    return sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npz"))


@pytest.mark.parametrize("name", fixtures())
def test_filter_and_filter_range_equal_the_reference(pipe, name):
    from urh_amd.filter import Filter, FilterType
    from urh_amd.signal import Signal
    z = np.load(os.path.join(GOLDEN_DIR, "dc", name + ".npz"), allow_pickle=False)
    iq = z["iq"]
    flt = Filter([], FilterType.dc_correction)
    assert same_bits(flt.work(dev(pipe, iq), pipe=pipe).cpu().numpy(), z["work"])
    assert same_bits(flt.work(iq, ctx=pipe.ctx), z["work"])
    sig = Signal(iq.copy(), pipe=pipe)
    sig.modulation_type = str(z["modulation_type"])
    sig.noise_threshold = float(z["noise_threshold"])
    _ = sig.qad
    sig.filter_range(int(z["start"]), int(z["end"]), flt)
    assert same_bits(sig.iq.cpu().numpy(), z["range_iq"])
    assert same_bits(np.ascontiguousarray(sig.qad_host(), np.float32), z["range_qad"])


def test_filter_range_still_takes_bare_taps_and_fir_filters(pipe, oracle):
    from urh_amd.filter import Filter, FilterType
    from urh_amd.signal import Signal
    iq = synth_fsk(20_000, sps=100, seed=3, noise=0.03)
    taps = (np.hanning(9) / np.hanning(9).sum()).astype(np.complex64)
    got = []
    for f in (taps, Filter(list(taps), FilterType.custom), Filter(list(taps), FilterType.moving_average)):
        sig = Signal(iq.copy(), pipe=pipe)
        sig.noise_threshold = 0.1
        _ = sig.qad
        sig.filter_range(1_001, 15_000, f)
        got.append((sig.iq.cpu().numpy(), np.array(sig.qad_host())))
    want = iq.copy()
    seg = np.ascontiguousarray(iq[1_001:15_000]).view(np.complex64).reshape(-1)
    want[1_001:15_000] = oracle.fir_filter(seg, taps).view(np.float32).reshape(-1, 2)
    for g_iq, g_qad in got:
        assert same_bits(g_iq, want) and same_bits(g_qad, got[0][1])
    y = Filter(list(taps)).work(dev(pipe, iq), pipe=pipe).cpu().numpy()
    assert same_bits(y, oracle.fir_filter(np.ascontiguousarray(iq).view(np.complex64).reshape(-1), taps).view(np.float32).reshape(-1, 2))


# ---- 3. the live sniffer ------------------------------------------------------------------------------------------------------------------
def bursts(n, sps, dtype, seed, chunk):
    """FSK bursts between silent gaps of at least three chunks (the sniffer flushes on a chunk of noise), on a DC term"""
    iq = synth_fsk(n, sps=sps, seed=seed, noise=0.02, pause_every=60 * sps, pause_len=max(25 * sps, 3 * chunk), dtype=np.float32)
    iq = iq * np.float32(0.5) + np.array([0.21, -0.13], np.float32)
    if np.dtype(dtype) == np.float32:
        return iq.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.round(iq * (info.max * 0.9)), info.min, info.max).astype(dtype)


@pytest.mark.parametrize("chunk", [1, 100, 8192, 32768])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=lambda d: np.dtype(d).name)
def test_live_sniffer_corrects_every_chunk(pipe, dtype, chunk):
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import LiveSniffer
    sps = {1: 4, 100: 10, 8192: 50, 32768: 100}[chunk]
    n = {1: 1_500, 100: 30_000, 8192: 200_000, 32768: 400_000}[chunk]
    iq = bursts(n, sps, dtype, seed=chunk, chunk=chunk)
    scale = 1.0 if dtype == np.float32 else float(np.iinfo(dtype).max)
    p = DemodParams("FSK", 1, 0.1 * scale, 0.0, 1.0, 2, sps, 0.1, 8, True)
    mine = LiveSniffer(pipe, p, dtype=dtype, buffer_samples=n + 16, clock=lambda: 100.0, trace=True, apply_dc_correction=True)
    ref = LiveSniffer(pipe, p, dtype=dtype, buffer_samples=n + 16, clock=lambda: 100.0, trace=True)
    for a in range(0, n, chunk):
        raw = iq[a:a + chunk]
        keep = raw.copy()
        mine.feed(raw if (a // chunk) % 2 else dev(pipe, raw))         # host arrays and device tensors alike
        assert same_bits(raw, keep)
        ref.feed(numpy_dc(raw)[0])
    assert mine.trace == ref.trace
    assert len(mine.messages) == len(ref.messages)
    if chunk >= 8192:
        assert len(ref.messages) > 0, "the capture produced no message: the case shows nothing"
    for a, b in zip(mine.messages, ref.messages):
        assert (a.plain_bits_str, a.pause, a.first_bit_sample_pos, a.timestamp) == (b.plain_bits_str, b.pause, b.first_bit_sample_pos, b.timestamp)


def test_live_sniffer_default_is_off(pipe):
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import LiveSniffer
    s = LiveSniffer(pipe, DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 10, 0.1, 8, True), buffer_samples=1000)
    assert s.engine.apply_dc_correction is False


# ---- 4. passes and capture streams --------------------------------------------------------------------------------------------------------
def ask_capture(n, sps, seed, dtype):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n // sps + 1)
    env = np.repeat(bits, sps)[:n].astype(np.float64)
    for a in range(20 * sps, n, 70 * sps):                       # on a fifth of the time: the corrected on and off levels stay apart
        env[a:a + 50 * sps] = 0
    iq = np.stack([env * 0.8, env * 0.3], axis=1) + 0.01 * rng.standard_normal((n, 2)) + (0.11, -0.07)
    if np.dtype(dtype) == np.float32:
        return iq.astype(np.float32)
    return np.round(iq * 20_000).astype(dtype)


def stream_case(kind):
    from urh_amd.pipeline import DemodParams
    if kind == "fsk":
        caps = [synth_fsk(n, sps=50, seed=n, noise=0.02, pause_every=3000, pause_len=1500) * np.float32(0.5) + np.array([0.2, 0.1], np.float32)
                for n in (30_011, 12_000, 40_000, 8_193, 25_000, 33_333)]
        return caps, DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 50, 0.1, 8, True), np.float32, {}
    if kind == "ask":
        caps = [ask_capture(n, 50, n, np.float32) for n in (30_011, 12_000, 40_000, 8_193, 25_000, 33_333)]
        return caps, DemodParams("ASK", 1, 0.2, 0.45, 1.0, 2, 50, 0.1, 8, True), np.float32, {}
    caps = [ask_capture(n, 50, n, np.int16) for n in (30_011, 12_000, 40_000, 8_193, 25_000, 33_333)]
    return caps, DemodParams("ASK", 1, 4000.0, 9000.0, 1.0, 2, 50, 0.1, 8, True), np.int16, {"auto_noise": True, "msg_records": True, "message_length_divisor": 4}


def summary(r, options):
    """what a stream handed out, copied out of the stream's pinned blocks"""
    s = [np.array(r.ppseq()), np.array(r.bits()), np.array(r.pauses)]
    if options.get("auto_noise"):
        s.append(np.array([r.noise_threshold, r.noise_flag], np.float64))
    if options.get("msg_records"):
        s.append(np.array(r.records).view(np.uint8))
    return s


def same_summaries(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["fsk", "ask", "ask_i16_auto_noise_records"])
def test_capture_stream_with_dc_correction(kind):
    """a stream with the option over raw captures == a stream without it over numpy-corrected captures, result by result; the caller's
    tensors are unchanged; no push of the warmed-up stream makes the host wait"""
    from urh_amd.pipeline import DevicePipeline
    caps, p, dtype, options = stream_case(kind)
    pipe = DevicePipeline(0)
    n_max = max(len(c) for c in caps)
    got = {}
    for corrected in (False, True):
        st = pipe.stream(n_max, p, want_qad=True, want_pos=True, dtype=dtype, dc_correction=not corrected, **options)
        tensors = [dev(pipe, numpy_dc(c)[0] if corrected else c) for c in caps]
        out = []
        before = None
        for k, t in enumerate(tensors):
            if k == 4:
                before = host_syncs()
            r = st.push(t)
            if r is not None:
                out.append(summary(r.check(), options))
        moved = host_syncs() - before
        for r in st.flush():
            out.append(summary(r.check(), options))
        st.close()
        assert len(out) == len(caps)
        got[corrected] = out
        if not corrected:
            assert moved == 0
            for t, c in zip(tensors, caps):
                assert same_bits(t.cpu().numpy(), c), "the caller's capture was modified"
    for k, (a, b) in enumerate(zip(got[False], got[True])):
        assert same_summaries(a, b), (kind, k)
    assert any(len(s[0]) > 10 for s in got[True]), "no pulse table to speak of: the case shows nothing"


@pytest.mark.parametrize("kind", ["fsk", "ask", "ask_i16_auto_noise_records"])
def test_one_pass_with_dc_correction(pipe, kind):
    caps, p, dtype, options = stream_case(kind)
    for k, c in enumerate(caps[:3]):
        raw = dev(pipe, c)
        mine = pipe.iq_to_bits(raw, p, want_qad=True, slot=k % 2, dc_correction=True, **options)
        a = [mine.ppseq(), *[np.asarray(v) for v in mine.flat()], mine.qad.cpu().numpy()]
        if options:
            a += [np.array([mine.noise_threshold, mine.noise_flag], np.float64), np.array(mine.records).view(np.uint8)]
        assert same_bits(raw.cpu().numpy(), c), "the caller's capture was modified"
        ref = pipe.iq_to_bits(dev(pipe, numpy_dc(c)[0]), p, want_qad=True, slot=k % 2, **options)
        b = [ref.ppseq(), *[np.asarray(v) for v in ref.flat()], ref.qad.cpu().numpy()]
        if options:
            b += [np.array([ref.noise_threshold, ref.noise_flag], np.float64), np.array(ref.records).view(np.uint8)]
        assert len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)), (kind, k)
        assert len(a[0]) > 10
