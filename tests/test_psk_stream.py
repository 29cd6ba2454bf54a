"""PSK in capture streams and on pipelined contexts (include/urhgpu.h: urhgpu_stream_*, tuning key "costas_dev_rounds"): the Costas
loop's re-speculation rounds are driven from the device, so a PSK pass queues like any other -- no stream synchronisation between its
kernels.  Every pass must equal the oracle (afp_demod with qad[0] = -4, grab_pulse_lens, ppseq_to_bits_flat) bit for bit, whatever is
in flight around it and however many rounds were queued."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from test_costas_shard import bits_equal, params, psk_capture

pytestmark = pytest.mark.gpu

# serial kernel / smallest parallel capture / three whole chunks / odd / several blocks of candidates / above 2^20 with a partial chunk
LENGTHS = (6_000, 8_200, 3 * 4096, 70_001, 240_000, (1 << 20) + 4096)
N_MAX = max(LENGTHS)
_refs = {}


def capture(order, i, dtype=np.float32):
    """capture i of the stream for `order` (seeded): its length drawn from LENGTHS, a gated gap in two captures of three"""
    rng = np.random.default_rng(1000 * order + i)
    n = int(LENGTHS[i] if i < len(LENGTHS) else rng.choice(LENGTHS))        # (every length at least once)
    gaps = () if i % 3 == 0 else ((n // 3, n // 3 + n // 7 + 300),)
    return psk_capture(n, order, seed=40 * order + i, dtype=dtype, gaps=gaps)


def reference(oracle, iq, p):
    """(qad, pulse table, bits, offsets, pauses, positions, position offsets) of the oracle"""
    qad = oracle.afp_demod(iq, p.noise_threshold, "PSK", 4 if p.bits_per_symbol == 2 else 2, p.costas_loop_bandwidth)
    qad[0] = -4.0                                           # the reference leaves it unwritten (np.empty)
    pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, "PSK", p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    return (qad, pp) + tuple(oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold))


def stream_refs(oracle, order):
    """the nine float32 captures of the stream for `order` with their references: computed once, shared, never changed"""
    if order not in _refs:
        caps = [capture(order, i) for i in range(9)]
        p = params(order, caps[0][1])
        _refs[order] = (caps, p, [reference(oracle, iq, p) for iq, _ in caps])
    return _refs[order]


def fetch_qad(pipe, r):
    out = np.empty(r.n_samples, np.float32)
    from urh_amd import _lib
    _lib.check(_lib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(r.d_qad_ptr), out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def host_syncs():
    from urh_amd import _lib
    return int(_lib.load().urhgpu_test_costas_host_syncs())


def run_stream(pipe, st, dev, with_qad=True, upload=None):
    """push every capture, flush; {seq: (qad or None, ppseq, bits, msg_off, pauses, pos, pos_off, n_samples)}"""
    got = {}

    def keep(r):
        if r is not None:
            r.check()
            qad = fetch_qad(pipe, r) if with_qad else None       # (valid until the next push)
            got[r.seq] = (qad, r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), r.bit_sample_pos(), r.pos_offsets(), r.n_samples)
    for k, d in enumerate(dev):
        keep(st.push(d) if upload is None else st.push_upload(upload[k], d))
    for r in st.flush():
        keep(r)
    return got


def assert_pass_equals(g, ref, what):
    qad, pp, bits, off, pauses, pos, poff = ref
    assert g[7] == len(qad), what
    if g[0] is not None:
        assert g[0][0] == -4.0 and bits_equal(g[0][1:], qad[1:]), (what, int((g[0][1:].view(np.uint32) != qad[1:].view(np.uint32)).sum()))
    assert np.array_equal(g[1], pp), what
    assert np.array_equal(g[2], bits) and np.array_equal(g[3], off) and np.array_equal(g[4], pauses), what
    assert np.array_equal(g[5], pos) and np.array_equal(g[6], poff), what


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("order", [2, 4])
def test_stream_of_different_psk_captures_equals_oracle(oracle, order, want_pos):
    import torch
    from urh_amd.pipeline import DevicePipeline
    caps, p0, refs = stream_refs(oracle, order)
    p = dataclasses.replace(p0, write_bit_sample_pos=want_pos)
    pipe = DevicePipeline(0)
    dev = [torch.from_numpy(iq).cuda() for iq, _ in caps]
    syncs0 = host_syncs()
    st = pipe.stream(N_MAX, p, want_qad=True, want_pos=want_pos)
    got = run_stream(pipe, st, dev)
    assert host_syncs() == syncs0                           # no pass waited for its own Costas rounds
    assert sorted(got) == list(range(len(caps)))
    for i, ref in enumerate(refs):
        assert_pass_equals(got[i], ref, (order, want_pos, i, len(caps[i][0])))
    stats = st.stats()["costas"]
    chunks = sum((len(iq) - 1 + 4095) // 4096 for iq, _ in caps if len(iq) > 8192)
    assert stats[0] + stats[1] + stats[2] == chunks - sum(1 for iq, _ in caps if len(iq) > 8192) and stats[3] == chunks, stats
    st.close()
    res = pipe.iq_to_bits(dev[0], p, want_qad=True)          # the pipeline is usable as before afterwards
    assert np.array_equal(res.ppseq(), refs[0][1])


@pytest.mark.parametrize("dtype", [np.int8, np.uint16])
def test_integer_psk_streams(oracle, dtype):
    import torch
    from urh_amd.pipeline import DevicePipeline
    caps = [psk_capture(n, 4, seed=77 + k, dtype=dtype, gaps=((n // 2, n // 2 + 3000),) if k else ()) for k, n in enumerate((8_200, 70_001, 3 * 4096))]
    p = params(4, caps[0][1])
    pipe = DevicePipeline(0)
    st = pipe.stream(70_001, p, want_qad=True, want_pos=True, dtype=dtype)
    got = run_stream(pipe, st, [torch.from_numpy(iq).cuda() for iq, _ in caps])
    st.close()
    for i, (iq, _) in enumerate(caps):
        assert_pass_equals(got[i], reference(oracle, iq, p), (np.dtype(dtype).name, i))


def noisy_capture(n=300_000, stretch=50_000):
    """order 4, a gated gap, and an un-gated noise-only stretch in which the loop wanders: the chunk chain breaks there"""
    iq, noise = psk_capture(n, 4, seed=5, gaps=((60_000, 90_000),))
    iq[150_000:150_000 + stretch] = (0.5 * np.random.default_rng(6).standard_normal((stretch, 2))).astype(np.float32)
    return iq, noise


def test_device_driven_rounds_equal_host_driven_rounds(oracle):
    import torch
    from urh_amd.pipeline import DevicePipeline
    iq, noise = noisy_capture()
    p = params(4, noise)
    ref = reference(oracle, iq, p)
    dev = torch.from_numpy(iq).cuda()
    chunks = (len(iq) - 1 + 4095) // 4096

    def one_shot(tuning):
        pipe = DevicePipeline(0, tuning=tuning)
        res = pipe.iq_to_bits(dev, p, want_qad=True)
        qad = res.qad.cpu().numpy()
        stats = pipe.ctx.costas_stats5()
        print("costas_dev_rounds", tuning, "stats", stats)
        assert bits_equal(qad[1:], ref[0][1:]) and np.array_equal(res.ppseq(), ref[1]), tuning
        assert stats[0] + stats[1] + stats[2] == chunks - 1 and stats[3] == chunks, (tuning, stats)
        return stats
    syncs0 = host_syncs()
    host = one_shot(None)
    assert host[4] >= 1, host                               # precondition: the host-driven path re-speculates on this capture
    assert host_syncs() - syncs0 == host[4] + 1             # one wait per round
    syncs0 = host_syncs()
    by_rounds = {r: one_shot({"costas_dev_rounds": r}) for r in (0, 1, 24)}
    assert host_syncs() == syncs0
    assert by_rounds[24] == host                            # the same sequence of rounds
    assert by_rounds[0][4] == 0 and by_rounds[0][2] > 0     # rounds exhausted: the chain was closed serially
    assert by_rounds[1][4] == 1


def test_psk_passes_do_not_synchronise_with_the_host():
    import torch
    from urh_amd.pipeline import DevicePipeline
    caps = [capture(4, i) for i in range(9)]
    p = params(4, caps[0][1])
    dev = [torch.from_numpy(iq).cuda() for iq, _ in caps]
    pipe = DevicePipeline(0)
    st = pipe.stream(N_MAX, p, want_qad=False, want_pos=True)
    before = host_syncs()
    got = run_stream(pipe, st, dev, with_qad=False)
    assert host_syncs() == before and len(got) == 9
    st.close()
    piped = DevicePipeline(0, pipelined=True)
    first = piped.iq_to_bits(dev[4], p, want_qad=True).ppseq().copy()
    assert host_syncs() == before
    assert np.array_equal(first, got[4][1])
    plain = DevicePipeline(0)
    assert np.array_equal(plain.iq_to_bits(dev[4], p, want_qad=True).ppseq(), got[4][1])
    assert host_syncs() > before                            # the default one-shot pass keeps the host-driven rounds


def test_push_upload_of_a_psk_capture(oracle):
    import torch
    from urh_amd.pipeline import DevicePipeline
    iq, noise = capture(4, 4)
    assert len(iq) == 240_000
    p = params(4, noise)
    pipe = DevicePipeline(0)
    st = pipe.stream(len(iq), p, want_qad=True, want_pos=True)
    pushed = run_stream(pipe, st, [torch.from_numpy(iq).cuda()])[0]
    host = torch.from_numpy(iq).pin_memory()
    dev = torch.empty_like(host, device="cuda")
    uploaded = run_stream(pipe, st, [dev], upload=[host])[1]
    st.close()
    assert np.array_equal(dev.cpu().numpy(), iq)
    assert bits_equal(uploaded[0], pushed[0])
    for a, b in zip(uploaded[1:], pushed[1:]):
        assert np.array_equal(a, b)
    assert_pass_equals(uploaded, stream_refs(oracle, 4)[2][4], "upload")


def test_from_file_streamed_takes_psk(tmp_path):
    from urh_amd.signal import Signal
    iq, noise = capture(4, 3)
    f = str(tmp_path / "psk.complex")
    iq.tofile(f)
    par = dict(modulation_type="PSK", bits_per_symbol=2, samples_per_symbol=100, center=0.0, center_spacing=1.5, tolerance=5, noise_threshold=noise,
               pause_threshold=8)
    s = Signal.from_file_streamed(f, **par)
    assert s.demod_passes == 1                               # the stream took it: no fall-back to the lazy passes
    ref = Signal.from_file(f)
    for k, v in par.items():
        setattr(ref, k, v)
    assert s.bits() == ref.bits() and len(s.bits()[0]) > 0
    assert s.demod_passes == 1
    assert bits_equal(s.qad.cpu().numpy(), ref.qad.cpu().numpy())
    assert np.array_equal(s.ppseq(), ref.ppseq())


def test_psk_and_fsk_streams_interleaved(oracle):
    import torch
    from conftest import synth_fsk
    from urh_amd.pipeline import DemodParams, DevicePipeline
    caps, p_psk, refs = stream_refs(oracle, 4)
    order = [5, 3, 4, 1, 2, 0]
    fsk = [synth_fsk(n, sps=100, seed=500 + k, noise=0.04, pause_every=n // 3, pause_len=n // 17 + 500) for k, n in enumerate((1 << 20, 70_001, 1 << 19, 1 << 20, 4096 * 3, 1 << 20))]
    p_fsk = DemodParams("FSK", 1, 0.1, 0.0, 1.0, 5, 100, 0.1, 8, True)
    pipes = DevicePipeline(0), DevicePipeline(0)
    st_psk = pipes[0].stream(N_MAX, p_psk, want_qad=True, want_pos=True)
    st_fsk = pipes[1].stream(1 << 20, p_fsk, want_qad=False, want_pos=True)
    d_psk = [torch.from_numpy(caps[i][0]).cuda() for i in order]
    d_fsk = [torch.from_numpy(c).cuda() for c in fsk]
    got_psk, got_fsk = {}, {}

    def keep(pipe, got, r, with_qad):
        if r is not None:
            r.check()
            got[r.seq] = (fetch_qad(pipe, r) if with_qad else None, r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), r.bit_sample_pos(), r.pos_offsets(),
                          r.n_samples)
    for a, b in zip(d_psk, d_fsk):
        keep(pipes[0], got_psk, st_psk.push(a), True)
        keep(pipes[1], got_fsk, st_fsk.push(b), False)
    for r in st_psk.flush():
        keep(pipes[0], got_psk, r, True)
    for r in st_fsk.flush():
        keep(pipes[1], got_fsk, r, False)
    st_psk.close()
    st_fsk.close()
    for k, i in enumerate(order):
        assert_pass_equals(got_psk[k], refs[i], ("psk", k))
    for k, iq in enumerate(fsk):
        qad = oracle.afp_demod(iq, 0.1, "FSK", 2)
        pp = oracle.grab_pulse_lens(qad, 0.0, 5, "FSK", 100, 1, 1.0)
        assert_pass_equals(got_fsk[k], (qad, pp) + tuple(oracle.ppseq_to_bits_flat(pp, 100, 1, True, 8)), ("fsk", k))
