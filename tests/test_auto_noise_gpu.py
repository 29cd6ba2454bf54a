"""The automatic noise threshold inside a pass, on the GPU: the chain alone (urhgpu_detect_noise_level_dev), one pass
(DevicePipeline.iq_to_bits(auto_noise=True), with and without auto_center), capture streams, the flags, Signal.from_file_streamed --
against the oracle (detect_noise_level -> afp_demod -> grab_pulse_lens -> _ppseq_to_bits) and against what the REAL reference recorded
in tests/golden/auto_noise.json.

One expectation is taken from the oracle rather than written down: a capture with ONE NaN sample in a quiet chunk.  There the chunk's mean
is a NaN, np.min of the means is a NaN, no chunk compares, np.max([]) raises ValueError inside detect_noise_level and it RETURNS 0
(AutoInterpretation.py:83-88; test_auto_noise_host.py::test_the_oracle_on_non_finite_captures pins this for the oracle, and the real
reference does the same) -- flag 1 with threshold 0, not an exception.  The test asserts whatever the oracle does with that capture, value
or exception; the exception at hand-out (flag 0) is exercised by an all-infinite capture, where math.ceil(inf) does raise."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import model_noise as mn
import noise_cases as nc

pytestmark = pytest.mark.gpu


def host_syncs():
    from urh_amd import _lib
    return int(_lib.load().urhgpu_test_noise_host_syncs())


def new_pipe(**kw):
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0, **kw)


@pytest.fixture(scope="module")
def pipe():
    return new_pipe()


@pytest.fixture(scope="module")
def piped():
    return new_pipe(pipelined=True)


@pytest.fixture(scope="module")
def gold():
    return nc.load_golden()


def to_dev(pipe, iq):
    import torch
    a = np.array(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(pipe.device).view(torch.uint16)
    return torch.from_numpy(a).to(pipe.device)


def chain(pipe, iq):
    """urhgpu_detect_noise_level_dev -> the result block; the call itself must not make the host wait"""
    import torch
    from urh_amd import _lib, signal_functions as sf
    lib = _lib.load()
    n = len(iq)
    dev = to_dev(pipe, iq) if n else None
    out = torch.zeros(C.sizeof(_lib.NoiseResult), dtype=torch.uint8, device=pipe.device)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    before = host_syncs()
    _lib.check(lib.urhgpu_detect_noise_level_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr() if n else None), sf.dtype_code(iq.dtype), n, C.c_void_p(out.data_ptr())))
    assert host_syncs() == before
    return _lib.NoiseResult.from_buffer_copy(out.cpu().numpy().tobytes())


# ---- 1. the chain alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", nc.DTYPES5, ids=lambda d: np.dtype(d).name)
def test_chain_alone_equals_detect_noise_level(oracle, pipe, dtype):
    for n in nc.CHAIN_SIZES:
        iq = nc.capture(7 + n, n, dtype=dtype)
        want, flag = nc.oracle_threshold(oracle, iq)
        r = chain(pipe, iq)
        what = (np.dtype(dtype).name, n, r.noise, want)
        print(*what)
        assert r.noise == want and r.flag == flag == 1, what
        assert (r.chunk, r.n_chunks) == mn.chunk_geometry(n), what
        assert r.noise_f32 == np.float32(want) and r.noise_sqrd == np.float32(np.float32(want) * np.float32(want)), what


def test_chain_on_short_and_degenerate_captures(oracle, pipe):
    for n in (0, 1, 3):
        r = chain(pipe, nc.capture(1, n))
        assert (r.noise, r.flag, r.n_chunks) == (0.0, 1, 0), n
    r = chain(pipe, np.zeros((20000, 2), np.float32))
    assert (r.noise, r.flag, r.n_candidates) == (0.0, 1, 0)
    const = nc.constant_envelope(20000)
    r = chain(pipe, const)
    assert (r.noise, r.flag) == (0.0, 1) and r.min_mean / r.max_mean > 0.9 and oracle.detect_noise_level(oracle.get_magnitudes(const)) == 0


def test_chain_reproduces_the_reference_fixture(pipe, gold):
    for name in ("size-12801", "size-300007", "gates-all", "pass-FSK2-int16", "pass-PSK4-int8"):
        g = gold[name]
        r = chain(pipe, nc.case_capture(g["recipe"]))
        assert r.noise == float.fromhex(g["threshold"]) and r.flag == (2 if g["gates_all"] else 1), (name, r.noise, r.flag)


# ---- 2. one pass -------------------------------------------------------------------------------------------------------------------
def outputs_of(res):
    res.check_capacity()
    return (res.ppseq(),) + tuple(res.flat())


def assert_pass(got_qad, got, ref, what):
    qad, pp, flat = ref
    if got_qad is not None:
        assert got_qad.shape == qad.shape and np.array_equal(got_qad.view(np.uint32), qad.view(np.uint32)), what
    assert np.array_equal(got[0], pp), what
    for k in range(5):                                                     # bits, message offsets, pauses, positions, position offsets
        assert np.array_equal(got[1 + k], flat[k]), (what, k)


@pytest.mark.parametrize("dtype", nc.PASS_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mod,bps", nc.PASS_MODS, ids=[f"{m}{1 << b}" for m, b in nc.PASS_MODS])
def test_one_pass_equals_oracle_and_fixture(oracle, pipe, piped, gold, mod, bps, dtype):
    g = gold[f"pass-{mod}{1 << bps}-{np.dtype(dtype).name}"]
    iq = nc.case_capture(g["recipe"])
    want, flag = nc.oracle_threshold(oracle, iq)
    assert flag == 1 and want == float.fromhex(g["threshold"])
    p = nc.params(mod, bps, noise=123.0)                                    # (the configured threshold must play no part)
    ref = nc.reference(oracle, iq, p, want)
    assert nc.messages_of(ref[2]) == (g["bits"], g["pauses"])               # the oracle's messages are the real reference's
    for name, pp in (("plain", pipe), ("pipelined", piped)):
        dev = to_dev(pp, iq)
        pp.iq_to_bits(dev, dataclasses.replace(p, noise_threshold=want), want_qad=True).check_capacity()      # (scratch of this shape in place)
        before = host_syncs()
        res = pp.iq_to_bits(dev, p, want_qad=True, auto_noise=True)
        if mod != "PSK" or name == "pipelined":                           # (PSK on a plain context keeps the host-driven Costas rounds)
            assert host_syncs() == before, (name, mod)
        assert res.noise_flag == 1 and res.noise_threshold == want, (name, res.noise_threshold, want)
        got = outputs_of(res)
        assert_pass(res.qad.cpu().numpy(), got, ref, (name, mod, bps, np.dtype(dtype).name))
        assert nc.messages_of(got[1:]) == (g["bits"], g["pauses"]), name


def test_one_pass_without_qad_and_on_a_partial_tile(oracle, pipe):
    """auto_noise alone needs no demodulated signal; a capture that ends inside a tile goes through the state-byte kernel too"""
    for n in (12801, 4099):
        iq = nc.capture(3000 + n % 7, n)
        want, _ = nc.oracle_threshold(oracle, iq)
        p = nc.params("FSK", 1)
        res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=False, auto_noise=True)
        assert res.noise_threshold == want
        assert_pass(None, outputs_of(res), nc.reference(oracle, iq, p, want), n)


def test_one_pass_with_eight_states(oracle, pipe):
    """order 8: the state-byte kernel reads the device threshold on every chunk"""
    iq = nc.capture(1011, nc.N_PASS, "FSK", 2)
    want, _ = nc.oracle_threshold(oracle, iq)
    p = dataclasses.replace(nc.params("FSK", 3), center_spacing=0.06)
    res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, auto_noise=True)
    assert res.noise_threshold == want
    assert_pass(res.qad.cpu().numpy(), outputs_of(res), nc.reference(oracle, iq, p, want), "order 8")


# ---- 3. auto_noise + auto_center -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", ["FSK", "ASK", "PSK"])
def test_noise_and_center_in_one_pass(oracle, pipe, piped, gold, mod):
    g = gold[f"pass-{mod}2-float32"]
    iq = nc.case_capture(g["recipe"])
    want = float.fromhex(g["threshold"])
    p = nc.params(mod, 1, noise=123.0)
    max_size = 150 * nc.SPS
    qad = nc.reference(oracle, iq, p, want)[0]
    c = oracle.detect_center(qad, max_size)
    assert c is not None
    ref = (qad,) + nc.slice_qad(oracle, qad, p, float(c))
    for name, pp in (("plain", pipe), ("pipelined", piped)):
        res = pp.iq_to_bits(to_dev(pp, iq), p, want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2, slot=5, auto_noise=True, auto_center=True,
                            center_max_size=max_size)
        assert res.noise_flag == 1 and res.noise_threshold == want
        assert res.center == float(c), (name, res.center, c, res.center_flag)     # (a tie, flag 3, is settled through the host path)
        assert_pass(res.qad.cpu().numpy(), outputs_of(res), ref, (name, mod))


# ---- 4. a stream of captures with their own noise floors ---------------------------------------------------------------------
_stream = {}


def stream_case(oracle, gold):
    if not _stream:
        caps = [nc.case_capture(gold[f"stream-{i}"]["recipe"]) for i in range(8)]
        thr = [float.fromhex(gold[f"stream-{i}"]["threshold"]) for i in range(8)]
        p = nc.params("FSK", 1, noise=0.02)
        refs = [nc.reference(oracle, iq, p, t) for iq, t in zip(caps, thr)]
        _stream.update(caps=caps, thr=thr, p=p, refs=refs)
    return _stream


def test_no_fixed_threshold_decodes_the_stream(oracle, gold):
    """what the stream test is about: whichever of the captures' thresholds is taken for all of them, some capture decodes differently"""
    s = stream_case(oracle, gold)
    for t in s["thr"] + [s["p"].noise_threshold]:
        wrong = [i for i, iq in enumerate(s["caps"]) if nc.messages_of(nc.reference(oracle, iq, s["p"], t)[2]) != nc.messages_of(s["refs"][i][2])]
        assert wrong, t
    assert max(s["thr"]) / min(s["thr"]) > 9


def fetch_qad(pipe, r):
    from urh_amd import _lib
    out = np.empty(r.n_samples, np.float32)
    _lib.check(_lib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(r.d_qad_ptr), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def run_stream(pipe, st, dev, upload=None, stop_before_flush=None, want_pos=True):
    got, order = {}, []

    def keep(r):
        if r is not None:
            r.check()
            order.append(r.seq)
            pos = (r.bit_sample_pos(), r.pos_offsets()) if want_pos else (None, None)
            got[r.seq] = (r.noise_threshold, r.noise_flag, fetch_qad(pipe, r), (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy()) + pos)
    for k, d in enumerate(dev):
        keep(st.push(d) if upload is None else st.push_upload(upload[k], d))
    if stop_before_flush is not None:
        stop_before_flush()
    for r in st.flush():
        keep(r)
    return got, order


@pytest.mark.parametrize("route", ["push", "push-no-pos", "push_upload"])
def test_stream_of_captures_with_their_own_thresholds(oracle, gold, route):
    import torch
    s = stream_case(oracle, gold)
    want_pos = route != "push-no-pos"
    p = dataclasses.replace(s["p"], write_bit_sample_pos=want_pos)
    pipe = new_pipe(pipelined=True)
    # each capture's one-shot pass
    one = []
    for iq in s["caps"]:
        res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, auto_noise=True)
        one.append((res.noise_threshold, res.qad.cpu().numpy(), outputs_of(res)))
    st = pipe.stream(max(nc.N_STREAM), p, want_qad=True, want_pos=want_pos, auto_noise=True)
    if route == "push_upload":
        host = [torch.from_numpy(np.array(iq)).pin_memory() for iq in s["caps"]]
        dev = [torch.empty_like(h, device=pipe.device) for h in host]
    else:
        host, dev = None, [to_dev(pipe, iq) for iq in s["caps"]]
    before = host_syncs()
    moved = []
    got, order = run_stream(pipe, st, dev, upload=host, stop_before_flush=lambda: moved.append(host_syncs() - before), want_pos=want_pos)
    assert moved == [0], moved                                             # no push made the host wait (the flush does not count)
    st.close()
    assert order == list(range(8))                                         # results in push order
    for i in range(8):
        noise, flag, qad, out = got[i]
        assert flag == 1 and noise == s["thr"][i] == one[i][0], (route, i, noise, s["thr"][i])
        assert np.array_equal(qad.view(np.uint32), one[i][1].view(np.uint32)), (route, i)
        for k in range(4 if not want_pos else 6):
            assert np.array_equal(out[k], one[i][2][k]), (route, i, k)
        ref = s["refs"][i]
        assert np.array_equal(out[0], ref[1]) and np.array_equal(out[1], ref[2][0]) and np.array_equal(out[3], ref[2][2]), (route, i)
        if route == "push_upload":
            assert np.array_equal(dev[i].cpu().numpy(), s["caps"][i])


def test_stream_of_integer_captures_with_the_probe(oracle):
    """int16 2-FSK: the stream's wide-deviation probe runs behind every pass, gated by the device threshold; results as one by one"""
    caps = [nc.capture(6000 + i, 16384 + 4096 * (i % 2), dtype=np.int16) for i in range(5)]
    p = nc.params("FSK", 1)
    pipe = new_pipe(pipelined=True)
    st = pipe.stream(20480, p, want_qad=True, want_pos=True, dtype=np.int16, auto_noise=True)
    got, order = run_stream(pipe, st, [to_dev(pipe, iq) for iq in caps])
    st.close()
    assert order == list(range(5))
    for i, iq in enumerate(caps):
        want, flag = nc.oracle_threshold(oracle, iq)
        ref = nc.reference(oracle, iq, p, want)
        assert got[i][:2] == (want, flag)
        assert np.array_equal(got[i][2].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[i][3][0], ref[1]), i


def test_stream_with_noise_and_center(oracle, gold):
    s = stream_case(oracle, gold)
    pipe = new_pipe(pipelined=True)
    p = s["p"]
    st = pipe.stream(max(nc.N_STREAM), p, want_qad=True, want_pos=True, auto_noise=True, auto_center=True, center_max_size=15000)
    got = {}
    for r in [st.push(to_dev(pipe, iq)) for iq in s["caps"][:4]] + st.flush():
        if r is not None:
            got[r.seq] = (r.noise_threshold, r.center, r.ppseq())
    st.close()
    for i in range(4):
        qad = s["refs"][i][0]
        c = oracle.detect_center(qad, 15000)
        assert got[i][0] == s["thr"][i] and got[i][1] == (None if c is None else float(c)), i
        assert np.array_equal(got[i][2], nc.slice_qad(oracle, qad, p, None if c is None else float(c))[0]), i


# ---- 5. flags ----------------------------------------------------------------------------------------------------------------------
def zeros2_result(oracle, p):
    """what the reference makes of quad_demod's zeros(2)"""
    return nc.slice_qad(oracle, np.zeros(2, np.float32), p)


def wide_tables(res):
    """the pass's wide device tables as it left them (before anything is settled at hand-out)"""
    c = res.counts.cpu().numpy()
    n_rows, n_msg, n_bits = int(c[0]), int(c[1]), int(c[2])
    return res.rows_buf[:n_rows].cpu().numpy(), res.bits_buf[:n_bits].cpu().numpy(), res.pauses_buf[:n_msg].cpu().numpy(), res.qad.cpu().numpy()


def test_flag_2_gives_the_zeros2_result(oracle, pipe, gold):
    g = gold["gates-all"]
    iq = nc.case_capture(g["recipe"])
    want = float.fromhex(g["threshold"])
    assert g["gates_all"] and want >= math.sqrt(2)
    p = nc.params("FSK", 1, noise=0.7)
    dev = to_dev(pipe, iq)
    cap_rows = len(iq) // (p.tolerance + 1) + 2                             # (a noise-dominated capture: the exact row bound)
    res = pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=cap_rows, slot=1, auto_noise=True)
    assert res.noise_flag == 2
    # the queued pass used the configured threshold: its wide outputs are those of the pass without auto_noise
    plain = pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=cap_rows, slot=2)
    plain.check_capacity()
    for a, b in zip(wide_tables(res), wide_tables(plain)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # at hand-out: the reference's zeros(2) result
    assert res.noise_threshold == want
    pp, flat = zeros2_result(oracle, p)
    got = outputs_of(res)
    assert np.array_equal(got[0], pp) and all(np.array_equal(got[1 + k], flat[k]) for k in range(5))
    assert nc.messages_of(got[1:]) == (g["bits"], g["pauses"])
    assert res.qad.cpu().numpy().tolist() == [0.0, 0.0]


def test_flag_2_in_the_middle_of_a_stream(oracle, gold):
    s = stream_case(oracle, gold)
    loud = nc.case_capture(dict(gold["gates-all"]["recipe"], n=20011))
    want, flag = nc.oracle_threshold(oracle, loud)
    assert flag == 2
    caps = [s["caps"][0], s["caps"][1], loud, s["caps"][3], s["caps"][4]]
    pipe = new_pipe(pipelined=True)
    p = s["p"]
    st = pipe.stream(max(nc.N_STREAM), p, want_qad=True, want_pos=True, auto_noise=True)
    got, order = run_stream(pipe, st, [to_dev(pipe, iq) for iq in caps])
    st.close()
    assert order == [0, 1, 2, 3, 4]
    pp, flat = zeros2_result(oracle, p)
    assert got[2][:2] == (want, 2) and np.array_equal(got[2][3][0], pp) and np.array_equal(got[2][3][1], flat[0])
    for k, i in ((0, 0), (1, 1), (3, 3), (4, 4)):
        assert got[k][:2] == (s["thr"][i], 1) and np.array_equal(got[k][3][0], s["refs"][i][1]), k


def test_a_nan_sample_in_a_quiet_chunk(oracle, pipe):
    """see the module's docstring: the expectation is the oracle's, value or exception"""
    iq = np.array(nc.capture(11, 60000))
    iq[100, 0] = np.nan
    want, flag = nc.oracle_threshold(oracle, iq)
    print("oracle:", want, flag)
    p = nc.params("FSK", 1, noise=0.02)
    res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, auto_noise=True)
    assert res.noise_flag == flag
    if flag == 0:
        with pytest.raises(type(want)):
            res.noise_threshold
        with pytest.raises(type(want)):
            res.ppseq()
    else:
        assert res.noise_threshold == want
        assert_pass(None, outputs_of(res), nc.reference(oracle, iq, p, want), "nan")


def test_flag_0_raises_at_hand_out(oracle, pipe):
    """an all-infinite capture: detect_noise_level reaches math.ceil(inf) -- OverflowError, flag 0; the queued pass used the configured threshold"""
    iq = np.full((20000, 2), np.inf, np.float32)
    want, flag = nc.oracle_threshold(oracle, iq)
    assert flag == 0 and isinstance(want, OverflowError)
    p = nc.params("ASK", 1, noise=0.02)
    dev = to_dev(pipe, iq)
    res = pipe.iq_to_bits(dev, p, want_qad=True, slot=1, auto_noise=True)
    assert res.noise_flag == 0
    plain = pipe.iq_to_bits(dev, p, want_qad=True, slot=2)
    plain.check_capacity()
    for a, b in zip(wide_tables(res), wide_tables(plain)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    with pytest.raises(OverflowError):
        res.noise_threshold
    with pytest.raises(OverflowError):
        res.ppseq()
    # ... and in a stream: at the hand-out, the other results finalised
    sp = new_pipe(pipelined=True)
    st = sp.stream(20000, p, want_qad=True, want_pos=True, auto_noise=True)
    quiet = nc.capture(12, 20000, "ASK")
    assert st.push(to_dev(sp, quiet)) is None and st.push(to_dev(sp, iq)) is None
    with pytest.raises(OverflowError) as exc:
        st.flush()
    st.close()
    results = exc.value.results
    assert results[1] is None and results[0].noise_threshold == nc.oracle_threshold(oracle, quiet)[0]


def test_constant_envelope_gives_threshold_0(oracle, pipe):
    iq = nc.constant_envelope(60000)
    p = nc.params("FSK", 1, noise=0.3)
    res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, auto_noise=True)
    assert (res.noise_threshold, res.noise_flag) == (0.0, 1)
    assert_pass(res.qad.cpu().numpy(), outputs_of(res), nc.reference(oracle, iq, p, 0.0), "constant envelope")


# ---- 6. Signal.from_file_streamed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ext", [("file-float32", ".complex"), ("file-int8", ".cs8")])
def test_signal_from_file_streamed_automatic(gold, tmp_path, name, ext):
    from urh_amd.signal import Signal
    g = gold[name]
    iq = nc.case_capture(g["recipe"])
    path = str(tmp_path / ("capture" + ext))
    np.array(iq).tofile(path)
    p = nc.params("FSK", 1)
    kw = dict(modulation_type="FSK", samples_per_symbol=p.samples_per_symbol, center=p.center, tolerance=p.tolerance, pause_threshold=p.pause_threshold)
    a = Signal.from_file(path, default_noise_threshold="automatic")
    for k, v in kw.items():
        setattr(a, k, v)
    want = a.get_protocol()
    s = Signal.from_file_streamed(path, default_noise_threshold="automatic", **kw)
    assert s.noise_threshold == a.noise_threshold == float.fromhex(g["threshold"])
    passes = s.demod_passes
    got = s.get_protocol()
    assert s.demod_passes == passes                                        # the streamed pass left the digitisation behind
    assert [dataclasses.astuple(m) for m in got] == [dataclasses.astuple(m) for m in want]
    assert [m.plain_bits_str for m in got] == g["bits"] and [int(m.pause) for m in got] == g["pauses"]
    # captures the streamed route cannot take fall back, the threshold detected the ordinary way
    f = Signal.from_file_streamed(path, default_noise_threshold="automatic", **dict(kw, modulation_type="ASK"))
    assert f.noise_threshold == a.noise_threshold


def test_without_auto_noise_the_entry_point_is_the_existing_pass(pipe, gold):
    """auto_noise = 0: urhgpu_iq_to_bits_auto_dev is urhgpu_iq_to_bits_dev / urhgpu_iq_to_bits_auto_center_dev"""
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    iq = nc.case_capture(gold["pass-FSK2-float32"]["recipe"])
    p = nc.params("FSK", 1, noise=0.05)
    dev, cp = to_dev(pipe, iq), p.to_c(np.float32)
    cap = int(lib.urhgpu_center_hist_cap(pipe.ctx.handle))
    block = torch.zeros(C.sizeof(_lib.CenterResult) + 4 * cap, dtype=torch.uint8, device=pipe.device)
    for auto_center in (0, 1):
        # (compared as the passes left their tables: a center the host settles at hand-out would replace them)
        want = pipe.iq_to_bits(dev, p, want_qad=True, slot=1, auto_center=bool(auto_center), center_max_size=15000)
        other = pipe.iq_to_bits(dev, dataclasses.replace(p, center=0.3), want_qad=True, slot=2)      # (another result in slot 2's buffers)
        other.check_capacity()
        assert not np.array_equal(wide_tables(other)[0], wide_tables(want)[0])
        _lib.check(lib.urhgpu_iq_to_bits_auto_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), len(iq), C.byref(cp), 0, auto_center, 15000,
                                                  C.byref(other._outputs), None, None, C.c_void_p(block.data_ptr()), None, cap))
        pipe.ctx.join()
        for a, b in zip(wide_tables(other), wide_tables(want)):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), auto_center


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors(pipe):
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    p = nc.params("FSK", 1)
    st = pipe.stream(8192, p, want_qad=True)
    st.push(torch.zeros((4096, 2), dtype=torch.float32, device=pipe.device))
    assert lib.urhgpu_stream_set_auto_noise(st._h, 1) == _lib.ERR_ARG       # after the first push
    st.flush()
    st.close()
    cp = p.to_c(np.float32)
    dev = torch.zeros((4096, 2), dtype=torch.float32, device=pipe.device)
    rows, counts, nres, cres = (torch.zeros(k, dtype=torch.int64, device=pipe.device) for k in (64, 8, 8, 8))
    o = _lib.Outputs()
    o.rows, o.cap_rows, o.counts = rows.data_ptr(), 32, counts.data_ptr()
    for auto_noise in (0, 1):                                              # auto_center without the demodulated signal, as today
        assert lib.urhgpu_iq_to_bits_auto_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), 4096, C.byref(cp), auto_noise, 1, -1, C.byref(o),
                                              C.c_void_p(nres.data_ptr()), None, C.c_void_p(cres.data_ptr()), None, 0) == _lib.ERR_ARG
    assert lib.urhgpu_iq_to_bits_auto_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), 4096, C.byref(cp), 1, 0, -1, C.byref(o), None, None, None, None,
                                          0) == _lib.ERR_ARG               # auto_noise without a result block
    with pytest.raises(ValueError):
        pipe.iq_to_bits(dev, p, want_qad=False, auto_noise=True, auto_center=True)
