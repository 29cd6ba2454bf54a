"""Automatic center inside a pass, on the GPU: the center chain alone (urhgpu_detect_center_dev), one pass
(DevicePipeline.iq_to_bits(auto_center=True)), capture streams and the live sniffer, each against the oracle: afp_demod (PSK: qad[0] =
-4.0), detect_center(qad, max_size), grab_pulse_lens with that center (the configured one where there is none), ppseq_to_bits_flat.
Every test also asserts the flag the device REPORTS against the outcome numpy expects (center_cases.expected), so that nothing passes
through the host fallback unnoticed.  The sweep (center_cases.py): 10 lengths around the chain's tiles (4096), leaves (128) and pairwise
pieces (8192), the five sample types (signed: gated gaps -- compaction and the first-sample skip; unsigned: nothing gated), FSK and ASK,
max_size None / 7500 / 1000 / 127."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import center_cases as cc
from conftest import synth_fsk

pytestmark = pytest.mark.gpu

COMBOS = [(mod, dt) for mod in cc.MODS for dt in cc.DTYPES]
IDS = [f"{mod}-{np.dtype(dt).name}" for mod, dt in COMBOS]


def host_syncs():
    from urh_amd import _lib
    return int(_lib.load().urhgpu_test_center_host_syncs())


def new_pipe(**kw):
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0, **kw)


@pytest.fixture(scope="module")
def pipe():
    return new_pipe()


def chain(pipe, qad, max_size, scratch_in_place=False):
    """urhgpu_detect_center_dev on a demodulated signal: (flag, center, n_bins, e0, delta, counts or None).  scratch_in_place: a longer signal
    has been through the pipe, so the call must not make the host wait (scratch that grows waits for the device, and is counted)"""
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    cap = int(lib.urhgpu_center_hist_cap(pipe.ctx.handle))
    d = torch.from_numpy(np.array(qad)).to(pipe.device) if len(qad) else torch.empty(0, dtype=torch.float32, device=pipe.device)
    out = torch.zeros(64 + 4 * cap, dtype=torch.uint8, device=pipe.device)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    before = host_syncs()
    _lib.check(lib.urhgpu_detect_center_dev(pipe.ctx.handle, C.c_void_p(d.data_ptr() if len(qad) else None), len(qad), -1 if max_size is None else max_size,
                                            C.c_void_p(out.data_ptr()), cap))
    assert not scratch_in_place or host_syncs() == before
    raw = out.cpu().numpy()
    r = _lib.CenterResult.from_buffer_copy(raw[:64].tobytes())
    counts = raw[64:64 + 4 * r.n_counts].view(np.uint32).astype(np.int64) if r.n_counts else None
    return int(r.flag), float(r.center), int(r.n_bins), float(r.e0), float(r.delta), counts


def check_chain(oracle, pipe, qad, max_size, what, pool_bins=cc.POOL_BINS, scratch_in_place=False):
    from urh_amd import estimators
    kind = cc.expected(qad, max_size, pool_bins)
    flag, center, nb, e0, delta, counts = chain(pipe, qad, max_size, scratch_in_place)
    assert flag == cc.FLAG[kind], (what, kind, flag)
    want = oracle.detect_center(qad, max_size)
    if kind == "ok":
        assert center == float(want), (what, center, want)
    elif kind == "none":
        assert want is None, what
    elif kind == "tie":
        y, x = cc.histogram(qad, max_size)
        assert nb == len(y) and np.array_equal(counts, y), what
        edges = e0 + np.arange(nb + 1, dtype=np.float64) * delta
        assert np.array_equal(edges, x), what
        assert float(estimators.peaks_center(counts, edges)) == float(want), what
    return kind


@pytest.mark.parametrize("mod,dtype", COMBOS, ids=IDS)
def test_chain_alone_equals_detect_center(oracle, pipe, mod, dtype):
    kinds = []
    chain(pipe, cc.sweep_qad(oracle, max(cc.LENGTHS), dtype, mod), None)          # the longest signal first: the scratch is in place from here on
    for n in cc.LENGTHS:
        qad = cc.sweep_qad(oracle, n, dtype, mod)
        for ms in cc.MAX_SIZES:
            kinds.append(check_chain(oracle, pipe, qad, ms, (mod, np.dtype(dtype).name, n, ms), scratch_in_place=True))
    print(mod, np.dtype(dtype).name, {k: kinds.count(k) for k in set(kinds)})


def test_chain_edge_cases(oracle, pipe):
    qad = cc.sweep_qad(oracle, 8193, np.float32, "FSK")
    assert check_chain(oracle, pipe, qad, 0, "max_size 0") == "none"
    kept = int((qad > -4).sum())
    flag, center = chain(pipe, qad, kept + 5)[:2]                                   # larger than the kept count: no cut
    assert flag == 1 and center == float(oracle.detect_center(qad, None)) == float(oracle.detect_center(qad, kept + 5))
    gated = oracle.afp_demod(cc.capture(8193, np.float32), 10.0, "FSK", 2)            # every sample below the noise gate
    assert not (gated > -4).any() and check_chain(oracle, pipe, gated, None, "all gated") == "none"
    const = oracle.afp_demod(np.full((5000, 2), 0.5, np.float32), 0.1, "ASK", 2)      # constant magnitude: zero variance
    assert check_chain(oracle, pipe, const, None, "constant ASK") == "none"
    assert check_chain(oracle, pipe, np.zeros(0, np.float32), None, "empty") == "none"
    assert check_chain(oracle, pipe, np.full(1, 0.3, np.float32), None, "one sample") == "none"


def test_chain_reports_a_histogram_beyond_the_pool(oracle):
    small = new_pipe(tuning={"auto_center_max_bins": 8})
    qad = cc.sweep_qad(oracle, 12289, np.int16, "FSK")
    assert len(cc.histogram(qad, 7500)[0]) > 8
    assert check_chain(oracle, small, qad, 7500, "forced wide", pool_bins=8) == "wide"


def one_pass(pipe, dev, p, max_size):
    res = pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=dev.shape[0] // (p.tolerance + 1) + 2, auto_center=True, center_max_size=max_size)
    flag, center = res.center_flag, res.center
    res.check_capacity()
    return flag, center, res.qad.cpu().numpy(), (res.ppseq(),) + tuple(res.flat())


@pytest.mark.parametrize("mod,dtype", COMBOS, ids=IDS)
def test_one_pass_equals_oracle(oracle, pipe, mod, dtype):
    import torch
    p = cc.params(mod, dtype)
    # the largest capture first: scratch and descriptor memory grow on the first pass that needs them, and growing waits for the device
    one_pass(pipe, torch.from_numpy(np.array(cc.capture(max(cc.LENGTHS), dtype))).to(pipe.device), p, None)
    for n in cc.LENGTHS:
        iq = cc.capture(n, dtype)
        dev = torch.from_numpy(np.array(iq)).to(pipe.device)
        key = (n, np.dtype(dtype).name, mod)
        for ms in cc.MAX_SIZES:
            what = (mod, np.dtype(dtype).name, n, ms)
            ref = cc.reference(oracle, iq, p, ms, key)
            kind = cc.expected(ref[1], ms)
            before = host_syncs()
            flag, center, qad, got = one_pass(pipe, dev, p, ms)
            assert flag == cc.FLAG[kind], (what, kind, flag)
            assert host_syncs() == before, what               # nothing below the pass's entry point made the host wait
            cc.assert_equal(center, qad, got, ref, what)


def test_one_pass_on_a_pipelined_context(oracle):
    """back-to-back auto_center passes on a pipelined context, read afterwards: slots of their own, results as one by one"""
    import torch
    piped = new_pipe(pipelined=True)
    p = cc.params("ASK", np.float32)
    cases = [(n, ms) for n in (4097, 70001, 20000) for ms in (None, 1000)]
    results = []
    for slot, (n, ms) in enumerate(cases):
        dev = torch.from_numpy(np.array(cc.capture(n, np.float32))).to(piped.device)
        results.append((dev, piped.iq_to_bits(dev, p, want_qad=True, cap_rows=n // 6 + 2, slot=slot + 1, auto_center=True, center_max_size=ms)))
    for (n, ms), (_, res) in zip(cases, results):
        ref = cc.reference(oracle, cc.capture(n, np.float32), p, ms, (n, "float32", "ASK"))
        assert res.center_flag == cc.FLAG[cc.expected(ref[1], ms)], (n, ms)
        cc.assert_equal(res.center, res.qad.cpu().numpy(), (res.ppseq(),) + tuple(res.flat()), ref, ("piped", n, ms))


@pytest.mark.parametrize("order", [2, 4])
def test_one_pass_psk(oracle, pipe, order):
    import torch
    from test_costas_shard import params as psk_params, psk_capture
    for n in (6000, 12288, 70001):
        for gaps in ((), ((n // 3, n // 3 + n // 7 + 300),)):
            iq, noise = psk_capture(n, order, seed=10 * order + len(gaps), gaps=gaps)
            p = psk_params(order, noise)
            dev = torch.from_numpy(np.array(iq)).to(pipe.device)
            for ms in (None, 7500):
                ref = cc.reference(oracle, iq, p, ms)
                kind = cc.expected(ref[1], ms)
                flag, center, qad, got = one_pass(pipe, dev, p, ms)
                assert flag == cc.FLAG[kind], (order, n, gaps, ms, kind, flag)
                assert qad[0] == -4.0
                cc.assert_equal(center, qad, got, ref, ("PSK", order, n, gaps, ms))


@pytest.mark.parametrize("bps,spacing", [(2, 0.1), (2, 0.45), (3, 0.05), (3, 0.15)])
def test_one_pass_with_several_thresholds_from_the_device(oracle, pipe, bps, spacing):
    """order 4: three thresholds in the bit-plane kernel (and the state-byte kernel on the partial tile); order 8: seven in the state-byte kernel"""
    import torch
    p = cc.params("FSK", np.float32, bits_per_symbol=bps, center_spacing=spacing)
    for n in (4097, 20000):
        iq = cc.capture(n, np.float32)
        ref = cc.reference(oracle, iq, p, 7500)
        kind = cc.expected(ref[1], 7500)
        flag, center, qad, got = one_pass(pipe, torch.from_numpy(np.array(iq)).to(pipe.device), p, 7500)
        assert flag == cc.FLAG[kind] == 1, (n, kind, flag)
        cc.assert_equal(center, qad, got, ref, (bps, n))


def test_one_pass_without_a_center_slices_with_the_configured_one(oracle, pipe):
    import torch
    p = cc.params("ASK", np.float32, noise=0.1)
    const = np.full((5000, 2), 0.5, np.float32)
    for iq, ms in ((const, None), (cc.capture(8193, np.float32), 0)):
        ref = cc.reference(oracle, iq, p, ms)
        assert ref[0] is None
        flag, center, qad, got = one_pass(pipe, torch.from_numpy(np.array(iq)).to(pipe.device), p, ms)
        assert flag == 0 and center is None
        cc.assert_equal(center, qad, got, ref, ("no center", ms))
        plain = pipe.iq_to_bits(torch.from_numpy(np.array(iq)).to(pipe.device), p, want_qad=True, slot=3)
        assert np.array_equal(plain.ppseq(), got[0])


def test_one_pass_settles_a_histogram_beyond_the_pool(oracle):
    import torch
    small = new_pipe(tuning={"auto_center_max_bins": 8})
    p = cc.params("FSK", np.int16)
    iq = cc.capture(12289, np.int16)
    ref = cc.reference(oracle, iq, p, 7500, (12289, "int16", "FSK"))
    assert cc.expected(ref[1], 7500, pool_bins=8) == "wide" and ref[0] is not None
    flag, center, qad, got = one_pass(small, torch.from_numpy(np.array(iq)).to(small.device), p, 7500)
    assert flag == 2
    cc.assert_equal(center, qad, got, ref, "forced wide")


# ---- capture streams -------------------------------------------------------------------------------------------------------
# nine captures, lengths of every residue of the three result slots and around the tiles; FSK: four of them at +-20 kHz deviation, seeded so that
# their second and third peaks tie at max_size 7500 (two of them back to back); ASK: amplitudes 0.3 .. 1.0, so the centers differ
# (captures of this family do not tie at 7500: ASK ties are covered by the one-pass sweep)
STREAM = ((4096, None), (20000, 3), (70001, None), (12289, 5), (8193, 6), (4097, None), (262221, None), (3000, None), (8191, 9))
N_MAX = 262221
_stream_refs = {}


def stream_case(oracle, mod):
    if mod not in _stream_refs:
        caps = []
        for k, (n, tie_seed) in enumerate(STREAM):
            if mod == "FSK":
                iq = cc.capture(n, np.float32) if tie_seed is None else synth_fsk(n, sps=cc.SPS, seed=tie_seed, noise=0.05, pause_every=2500, pause_len=700,
                                                                                   deviation_hz=20e3)
            else:
                iq = (cc.capture(n, np.float32) * np.float32(0.3 + 0.7 * k / 8)).astype(np.float32)
            caps.append(iq)
        p = cc.params(mod, np.float32, noise=0.3 if mod == "FSK" else 0.1)
        refs = [cc.reference(oracle, iq, p, 7500) for iq in caps]
        _stream_refs[mod] = (caps, p, refs, [cc.expected(r[1], 7500) for r in refs])
    return _stream_refs[mod]


def fetch_qad(pipe, r):
    from urh_amd import _lib
    out = np.empty(r.n_samples, np.float32)
    _lib.check(_lib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(r.d_qad_ptr), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def run_stream(pipe, st, dev, upload=None, stop_before_flush=None):
    got = {}

    def keep(r):
        if r is not None:
            r.check()
            got[r.seq] = (r.center, r.center_flag, fetch_qad(pipe, r), (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), r.bit_sample_pos(), r.pos_offsets()))
    for k, d in enumerate(dev):
        keep(st.push(d) if upload is None else st.push_upload(upload[k], d))
    if stop_before_flush is not None:
        stop_before_flush()
    for r in st.flush():
        keep(r)
    return got


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_stream_of_captures_with_their_own_centers(oracle, mod, want_pos):
    import torch
    caps, p0, refs, kinds = stream_case(oracle, mod)
    if mod == "FSK":
        assert kinds.count("tie") >= 3 and kinds[3] == kinds[4] == "tie", kinds
    else:
        assert kinds == ["ok"] * 9 and len({r[0] for r in refs}) == 9, kinds
    p = dataclasses.replace(p0, write_bit_sample_pos=want_pos)
    pipe = new_pipe(pipelined=True)
    dev = [torch.from_numpy(np.array(iq)).to(pipe.device) for iq in caps]
    st = pipe.stream(N_MAX, p, want_qad=True, want_pos=want_pos, auto_center=True, center_max_size=7500)
    before = host_syncs()
    moved = []
    got = run_stream(pipe, st, dev, stop_before_flush=lambda: moved.append(host_syncs() - before))
    # no pass of the stream made the host wait (its scratch was reserved by urhgpu_stream_set_auto_center); settling the ties at the
    # hand-out is not the pass
    assert moved == [0] and host_syncs() == before
    st.close()
    assert sorted(got) == list(range(9))
    for i, ref in enumerate(refs):
        center, flag, qad, out = got[i]
        assert flag == cc.FLAG[kinds[i]], (mod, i, kinds[i], flag)
        cc.assert_equal(center, qad, out, ref, (mod, want_pos, i))


def test_stream_push_upload(oracle):
    import torch
    caps, p, refs, kinds = stream_case(oracle, "FSK")
    pipe = new_pipe(pipelined=True)
    st = pipe.stream(N_MAX, p, want_qad=True, want_pos=True, auto_center=True, center_max_size=7500)
    host = [torch.from_numpy(np.array(iq)).pin_memory() for iq in caps[:5]]
    dev = [torch.empty_like(h, device=pipe.device) for h in host]
    got = run_stream(pipe, st, dev, upload=host)
    st.close()
    for i in range(5):
        assert np.array_equal(dev[i].cpu().numpy(), caps[i])
        center, flag, qad, out = got[i]
        assert flag == cc.FLAG[kinds[i]]
        cc.assert_equal(center, qad, out, refs[i], ("upload", i))


def test_pass_without_qad_is_an_argument_error(pipe):
    import torch
    from urh_amd import _lib
    p = cc.params("FSK", np.float32).to_c(np.float32)
    dev = torch.zeros((4096, 2), dtype=torch.float32, device=pipe.device)
    rows, counts, res = (torch.zeros(k, dtype=torch.int64, device=pipe.device) for k in (64, 8, 8))
    o = _lib.Outputs()
    o.rows, o.cap_rows, o.counts = rows.data_ptr(), 32, counts.data_ptr()
    call = lambda: _lib.load().urhgpu_iq_to_bits_auto_center_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), 4096, C.byref(p), -1, C.byref(o),
                                                                 C.c_void_p(res.data_ptr()), None, 0)
    assert call() == _lib.ERR_ARG                                # out->qad == NULL
    o.qad = torch.zeros(4096, dtype=torch.float32, device=pipe.device).data_ptr()
    o.blob, o.cap_blob = rows.data_ptr(), 64                     # a blob without the bit outputs: rejected before the pass begins
    assert call() == _lib.ERR_ARG


def test_stream_argument_errors(pipe):
    from urh_amd import _lib
    p = cc.params("FSK", np.float32)
    with pytest.raises(ValueError):
        pipe.stream(8192, p, want_qad=False, auto_center=True)
    st = pipe.stream(8192, p, want_qad=True)
    import torch
    st.push(torch.zeros((4096, 2), dtype=torch.float32, device=pipe.device))
    assert _lib.load().urhgpu_stream_set_auto_center(st._h, 1, 100) == _lib.ERR_ARG      # after the first push
    st.flush()
    st.close()


# ---- the live sniffer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ask_f32_autocenter", "fsk_f32_adaptive_autocenter"])
def test_sniffer_with_automatic_center(oracle, pipe, name):
    """the recorded runs with automatic_center: the messages and centers as recorded, every flush ONE queued pass -- a flush whose
    center the device decides makes the host wait once at most below the pass's entry point (urhgpu_test_center_host_syncs)"""
    import model_sniffer as msn
    from urh_amd.sniffer import GpuSniffEngine
    g = msn.load_case(name)
    assert g["automatic_center"]
    flushes = []

    class Counting(GpuSniffEngine):
        def flush(self, index, params, automatic_center):
            iq = self.buffer[:index].cpu().numpy()
            qad = oracle.afp_demod(iq, params.noise_threshold, params.modulation_type, 2 ** params.bits_per_symbol)
            kind = cc.expected(qad, 150 * params.samples_per_symbol)
            before = host_syncs()
            out = super().flush(index, params, automatic_center)
            flushes.append((kind, host_syncs() - before))
            return out
    engine = Counting(pipe, g["iq"].dtype, g["buffer_samples"])
    sniffer = msn.make_sniffer(g, engine, pipe)
    # one pass over the whole (zeroed) buffer first: scratch and descriptor memory grow on the first pass that needs them, which waits for the device
    engine.buffer.zero_()
    n_buf, par = int(engine.buffer.shape[0]), sniffer.params
    pipe.iq_to_bits(engine.buffer, par, want_qad=True, cap_rows=n_buf // (par.tolerance + 1) + 2, auto_center=True,
                    center_max_size=150 * par.samples_per_symbol).host_counts()
    msn.check_against_fixture(g, sniffer, msn.chunks_of(g))
    assert len(flushes) == len(g["centers"]) >= 1
    print(name, flushes)
    for kind, waits in flushes:
        assert kind != "ok" or waits <= 1, flushes
