"""The demodulation and pulse-table kernels on edge VALUES (tests/edge_inputs.py): NaN / inf / extreme floats inside batches that are
otherwise in the fast loop's window, amplitudes scaled to the window's bounds (2^+-40) and beyond under- and overflow, samples exactly
on the noise gate (`<=`: a tie is NOISE), NaN / inf / threshold-equal values in the demodulated signal.  Every case is compared with the
oracle -- which tests/test_edge_values_host.py pins to the real reference on the same inputs --: qad by bits (NaN with NaN equal), the
pulse table, bits, offsets, pauses and bit_sample_pos exactly.  Entry points: the one-shot fused pass under every chunk plan / tail
form, the wide loop, the host API, the speculative Costas loop (host- and device-driven rounds), capture streams, shards, segmentation."""
import contextlib

import numpy as np
import pytest

import edge_inputs as E

pytestmark = pytest.mark.gpu

TOL, PAUSE = 3, 8
PLANS = (None, "tiles", "generic_tail", "state_bytes")
_refs = {}


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def sf():
    from urh_amd import signal_functions
    return signal_functions


@contextlib.contextmanager
def forced(plan):
    """one of the library's test hooks for the duration of a pass, restored whatever happens"""
    from urh_amd import _lib
    lib = _lib.load()
    hooks = {"tiles": (lib.urhgpu_test_force_tiles_per_chunk, 4), "generic_tail": (lib.urhgpu_test_force_generic_tail, 1),
             "state_bytes": (lib.urhgpu_test_force_state_bytes, 1)}
    try:
        if plan is not None:
            hooks[plan][0](hooks[plan][1])
        yield
    finally:
        if plan is not None:
            hooks[plan][0](0)


def reference(oracle, key, iq, mod, bps, noise, center, spacing, sps, bw=0.1):
    """(qad, pulse table, (bits, offsets, pauses, positions, position offsets)) of the oracle: computed once per case, never changed"""
    if key not in _refs:
        with np.errstate(all="ignore"):
            qad = oracle.afp_demod(iq, noise, mod, 2 ** bps, bw)
        if mod == "PSK":
            qad[0] = -4.0                                   # the reference leaves it unwritten (np.empty)
        pp = oracle.grab_pulse_lens(qad, center, TOL, mod, sps, bps, spacing)
        _refs[key] = (qad, pp, oracle.ppseq_to_bits_flat(pp, sps, bps, True, PAUSE))
    return _refs[key]


def assert_qad(got, want, what):
    same = E.same_bits(got, want)
    bad = np.nonzero(~same)[0]
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:6], got[bad[:6]], want[bad[:6]])


def assert_result(res, ref, what, with_qad=True):
    qad, pp, flat = ref
    if with_qad:
        assert_qad(res.qad.cpu().numpy(), qad, what)
    assert np.array_equal(res.ppseq(), pp), (what, "pulse table")
    for k, (a, b) in enumerate(zip(flat, res.flat())):
        assert np.array_equal(a, b), (what, ("bits", "msg_off", "pauses", "pos", "pos_off")[k])


def params(mod, bps, noise, center, spacing, sps, bw=0.1):
    from urh_amd.pipeline import DemodParams
    return DemodParams(mod, bps, noise, center, spacing, TOL, sps, bw, PAUSE, True)


def run_fused(pipes, oracle, key, iq, mod, bps, noise, center, spacing, plans=PLANS):
    """the capture through iq_to_bits on every pipeline under every plan, and once for the bits alone"""
    import torch
    ref = reference(oracle, key, iq, mod, bps, noise, center, spacing, E.SPS)
    p = params(mod, bps, noise, center, spacing, E.SPS)
    dev = torch.from_numpy(iq).cuda()
    cap = len(iq) // (TOL + 1) + 2
    for k, pl in enumerate(pipes):
        for plan in plans:
            with forced(plan):
                res = pl.iq_to_bits(dev, p, want_qad=True, cap_rows=cap)
                assert_result(res, ref, (key, k, plan))
    res = pipes[0].iq_to_bits(dev, p, want_qad=False, cap_rows=cap)
    assert_result(res, ref, (key, "bits only"), with_qad=False)


# ---- one-shot fused pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_fused_pass_float_specials_and_scales(pipe, oracle, mod, bps):
    for tag, iq, noise, center, spacing in E.float_cases(mod, 2 ** bps):
        run_fused([pipe], oracle, (mod, bps, tag), iq, mod, bps, noise, center, spacing)


def test_fused_pass_wide_loop_specials_and_scales(pipe, oracle):
    """+-140 kHz steps (0.88 rad per sample): the batches sit in fsk_wide, whose window and hand-back to the generic step see the same values"""
    for tag, iq, noise, center, spacing in E.float_cases("FSK", 2, 140e3):
        run_fused([pipe], oracle, ("FSK wide", tag), iq, "FSK", 1, noise, center, spacing)


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_fused_pass_ties_on_the_gate(pipe, oracle, mod, dtype):
    from urh_amd.pipeline import DevicePipeline
    pipes = [pipe] + ([DevicePipeline(0, tuning={"wide_int": 1})] if np.dtype(dtype).kind == "i" else [])
    for bps in (1, 2) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.int16)) else (1,):
        for tag, iq, nt, center, spacing in E.tie_cases(mod, dtype, 2 ** bps):
            ref = reference(oracle, (mod, bps, np.dtype(dtype).name, tag), iq, mod, bps, nt, center, spacing, E.SPS)
            g = E.gate_classes(iq, nt)[1:]
            noise_val = oracle.noise_for_mod_type(mod)
            assert ((ref[0][1:] == noise_val) == (g <= 0)).all() and (g == 0).sum() >= 100          # the oracle gates the ties, and only gated samples
            run_fused(pipes, oracle, (mod, bps, np.dtype(dtype).name, tag), iq, mod, bps, nt, center, spacing)


def test_fused_pass_tie_at_threshold_zero(pipe, oracle):
    """noise_threshold = 0: a sample whose squares underflow to zero is a tie (0 <= 0: NOISE)"""
    iq, _ = E.base_capture("FSK")
    iq = E.sprinkle(iq, [500, 8192 + 127], [(E.SPECIALS["+1e-30"], E.SPECIALS["-1e-30"]), (E.SPECIALS["+1e-40"], E.SPECIALS["-0"])])
    for mod, center in (("FSK", 0.0), ("ASK", 0.4)):
        run_fused([pipe], oracle, (mod, "zero threshold"), iq, mod, 1, 0.0, center, 1.0)
        assert _refs[(mod, "zero threshold")][0][500] == oracle.noise_for_mod_type(mod)


# ---- host API: the streaming structure plus the k_afp_demod remainder, the pulse-table kernels -------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("mod", ["FSK", "ASK", "PSK"])
def test_host_afp_demod(sf, oracle, mod, order):
    bps = order.bit_length() - 1
    cases = [c[:3] for c in E.float_cases(mod, order)] + [c[:3] for dt in E.DTYPES for c in E.tie_cases(mod, dt, order)]
    if mod == "FSK":
        cases += [("wide " + c[0],) + c[1:3] for c in E.float_cases(mod, order, 140e3)]
    for tag, iq, noise in cases:
        with np.errstate(all="ignore"):
            want = oracle.afp_demod(iq, noise, mod, order)
        got = sf.afp_demod(iq, noise, mod, order)
        st = 1 if mod == "PSK" else 0
        assert_qad(got[st:], want[st:], (mod, order, bps, iq.dtype.name, tag))


@pytest.mark.parametrize("mod", ["FSK", "ASK", "PSK"])
def test_host_pulse_table_with_nan_inf_and_threshold_values(sf, oracle, mod):
    for order in (2, 4):
        x, center, spacing = E.rect_with_specials(order, mod)
        for bps in (1, 2):
            for tol in (2, 3):
                want = oracle.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing)
                got = sf.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing)
                assert np.array_equal(want, got), (mod, order, bps, tol, len(want), len(got))
                fb = oracle.ppseq_to_bits_flat(want, 40, bps, True, PAUSE)
                gb = sf.ppseq_to_bits_flat(got, 40, bps, True, PAUSE)
                assert all(np.array_equal(a, b) for a, b in zip(fb, gb)), (mod, order, bps, tol)
            if bps == order.bit_length() - 1:                # ... and a NaN run longer than the tolerance is a row of the TOP state
                assert (want[:, 0] == order - 1).any()


def test_fused_pass_slices_a_demodulated_signal_with_nan(pipe, oracle):
    """the bit-plane ballots and the state-byte kernel (qad_to_bits) on the same signals"""
    import torch
    from urh_amd import _lib
    from urh_amd.pipeline import DemodParams
    for mod in ("FSK", "ASK"):
        for order in (2, 4):
            bps = order.bit_length() - 1
            x, center, spacing = E.rect_with_specials(order, mod)
            pp = oracle.grab_pulse_lens(x, center, TOL, mod, 40, bps, spacing)
            flat = oracle.ppseq_to_bits_flat(pp, 40, bps, True, PAUSE)
            for plan in (None, "state_bytes"):
                with forced(plan):
                    res = pipe.qad_to_bits(torch.from_numpy(x).cuda(), DemodParams(mod, bps, 0.0, center, spacing, TOL, 40, 0.1, PAUSE, True))
                    assert np.array_equal(res.ppseq(), pp), (mod, order, plan)
                    assert all(np.array_equal(a, b) for a, b in zip(flat, res.flat())), (mod, order, plan)
    assert _lib.load().urhgpu_test_force_state_bytes(0) == 0


# ---- PSK: the speculative Costas loop -----------------------------------------------------------------------------------------------------
def psk_cases(order):
    tie, nt = E.tie_capture(np.float32)
    return E.float_cases("PSK", order) + [("tie", tie, nt, 0.0, 1.5 if order == 4 else 1.0)]


@pytest.mark.parametrize("rounds", [None, 24])
@pytest.mark.parametrize("bw", [0.1, 0.05])
@pytest.mark.parametrize("order", [2, 4])
def test_psk_fused_pass_on_the_speculative_path(oracle, order, bw, rounds):
    """rounds: None -- the host drives the re-speculation rounds; 24 -- they are queued and driven from the device"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    pl = DevicePipeline(0, tuning=None if rounds is None else {"costas_dev_rounds": rounds})
    bps = order.bit_length() - 1
    for tag, iq, noise, center, spacing in psk_cases(order):
        ref = reference(oracle, ("PSK", order, bw, tag), iq, "PSK", bps, noise, center, spacing, E.PSK_SPS, bw)
        res = pl.iq_to_bits(torch.from_numpy(iq).cuda(), params("PSK", bps, noise, center, spacing, E.PSK_SPS, bw), want_qad=True, cap_rows=len(iq) // (TOL + 1) + 2)
        assert_result(res, ref, ("PSK", order, bw, rounds, tag))
        stats = pl.ctx.costas_stats5()
        chunks = (len(iq) - 1 + 4095) // 4096
        print("PSK", order, bw, rounds, tag, "costas stats", stats)
        # the speculative path, not the serial kernel (whose stats are all zero): every chunk accounted for, the chain closed
        assert stats[0] + stats[1] + stats[2] == chunks - 1 and stats[3] == chunks, (order, bw, rounds, tag, stats)


# ---- capture streams ------------------------------------------------------------------------------------------------------------------------
def stream_captures(mod, dtype):
    """clean base, sprinkled, scaled by 2^-20 (everything gated at the stream's threshold) and by 2^20 (the window's upper bound), ties,
    the clean base again -- all at the tie capture's threshold, which gates the base capture's pause as well"""
    tie, nt = E.tie_capture(dtype)
    base, _ = E.base_capture(mod, dtype)
    if np.dtype(dtype) != np.float32:
        return [base, tie, base, tie, base], nt
    return [base, E.sprinkled(mod, 1)[0], E.scaled(base, -20), E.scaled(base, 20), tie, base], nt


@pytest.mark.parametrize("upload", [False, True])
@pytest.mark.parametrize("mod,dtype", [("FSK", np.float32), ("FSK", np.int8), ("PSK", np.float32)])
def test_capture_stream_with_edge_captures_between_clean_ones(oracle, mod, dtype, upload):
    import torch
    from test_psk_stream import run_stream
    from urh_amd.pipeline import DevicePipeline
    caps, nt = stream_captures(mod, dtype)
    sps = E.PSK_SPS if mod == "PSK" else E.SPS
    p = params(mod, 1, nt, 0.0, 1.0, sps)
    refs = [reference(oracle, ("stream", mod, np.dtype(dtype).name, k), iq, mod, 1, nt, 0.0, 1.0, sps) for k, iq in enumerate(caps)]
    pl = DevicePipeline(0)
    st = pl.stream(max(len(c) for c in caps), p, want_qad=True, want_pos=True, dtype=dtype, cap_rows=max(len(c) for c in caps) // (TOL + 1) + 2)
    try:
        if upload:
            host = [torch.from_numpy(c).pin_memory() for c in caps]
            got = run_stream(pl, st, [torch.empty_like(h, device="cuda") for h in host], upload=host)
        else:
            got = run_stream(pl, st, [torch.from_numpy(c).cuda() for c in caps])
    finally:
        st.close()
    assert sorted(got) == list(range(len(caps)))
    for k, (qad, pp, flat) in enumerate(refs):
        g = got[k]
        what = (mod, np.dtype(dtype).name, upload, k)
        assert g[7] == len(qad), what
        st0 = 1 if mod == "PSK" else 0
        assert_qad(g[0][st0:], qad[st0:], what)
        assert np.array_equal(g[1], pp), what
        assert all(np.array_equal(a, b) for a, b in zip(flat, g[2:7])), what
    # the clean capture after the edge captures equals the one before them: no state carried over from a NaN pass
    assert np.array_equal(got[0][0].view(np.uint32), got[len(caps) - 1][0].view(np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(got[0][1:7], got[len(caps) - 1][1:7]))


# ---- shards -----------------------------------------------------------------------------------------------------------------------------
def cuts_for(world, n):
    """cuts at multiples of 8, none of them on a chunk seam"""
    return [8192 * 2 + 64] if world == 2 else [8192 + 1024, min(3 * 8192 - 64, (n - 2000) // 8 * 8)]


def specials_at_cuts(iq, cuts, d, last_name="nan"):
    """a special d samples from every cut (d = -1: the last sample of a shard; 0: the first of the next; below -1: inside the halo);
    the last cut's is last_name, the others +-3e38 in one component"""
    names = ["+3e38", "-3e38"][:len(cuts) - 1] + [last_name]
    return E.sprinkle(iq, [c + d for c in cuts], [((E.SPECIALS[nm], None) if k % 2 == 0 else (None, E.SPECIALS[nm])) for k, nm in enumerate(names)])


def bounds_of(cuts, n):
    e = [0] + list(cuts) + [n]
    return [(e[r], e[r + 1]) for r in range(len(e) - 1)]


def check_fsk_shards(pipe, oracle, key, iq, mod, noise, center, bounds):
    import torch
    from test_sharding import run_threads
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import stitch
    n = len(iq)
    ref = reference(oracle, key, iq, mod, 1, noise, center, 1.0, E.SPS)
    p = params(mod, 1, noise, center, 1.0, E.SPS)
    dev = torch.from_numpy(iq).cuda()
    single = pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=n // (TOL + 1) + 2)
    assert_result(single, ref, (key, "single"))
    shards = [dev[a:b] for a, b in bounds]
    for halos in (None, [None] + [dev[a - 2:a].clone() for a, _ in bounds[1:]]):       # the halo exchanged / handed over with the shard
        res = run_threads(len(bounds), lambda r: GpuShardEngine(0), shards, bounds, n, p, halos)
        got = stitch(res)
        for k, (a, b) in enumerate(zip(got, (ref[1],) + tuple(ref[2]))):
            assert np.array_equal(a, b), (key, bounds, halos is not None, k)
        assert_qad(np.concatenate([r.qad.cpu().numpy() for r in res]), ref[0], (key, bounds, halos is not None))


@pytest.mark.parametrize("world", [2, 3])
def test_fsk_shards_with_a_special_at_the_cut(pipe, oracle, world):
    base, noise = E.base_capture("FSK")
    cuts = cuts_for(world, len(base))
    for d in (-1, 0, -2):
        for name in ("nan", "-inf"):
            iq = specials_at_cuts(base, cuts, d, name)
            check_fsk_shards(pipe, oracle, ("shard", "FSK", world, d, name), iq, "FSK", noise, 0.0, bounds_of(cuts, len(iq)))
    for dtype in (np.int8, np.float32):                          # a tie capture cut inside a run of ties
        iq, nt = E.tie_capture(dtype)
        runs = [(a, b) for a, b in E.tie_runs(iq, nt) if (a // 8 + 1) * 8 < b - 1 and a < (a // 8 + 1) * 8]
        picks = [runs[len(runs) * (k + 1) // (world + 1)] for k in range(world - 1)]
        tcuts = [(a // 8 + 1) * 8 for a, _ in picks]
        g = E.gate_classes(iq, nt)
        assert all(g[c - 1] == 0 and g[c] == 0 for c in tcuts)
        check_fsk_shards(pipe, oracle, ("shard tie", world, np.dtype(dtype).name), iq, "FSK", nt, 0.0, bounds_of(tcuts, len(iq)))


@pytest.mark.parametrize("world", [2, 3])
def test_psk_shards_with_a_special_at_the_cut(pipe, oracle, world):
    import torch
    from test_costas_shard import run_sharded
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import costas_halo_samples, stitch
    engines = [GpuShardEngine(0) for _ in range(world)]
    base, noise = E.base_capture("PSK", order=4)
    n = len(base)
    cuts = [22528] if world == 2 else [8200, 22528]              # the last cut in the capture's last tenth: the NaN goes there
    tie, nt = E.tie_capture(np.float32)
    runs = [(a, b) for a, b in E.tie_runs(tie, nt) if a < (a // 8 + 1) * 8 < b - 1]
    tcuts = [(runs[len(runs) * (k + 1) // (world + 1)][0] // 8 + 1) * 8 for k in range(world - 1)]
    cases = [(("shard", "PSK", world, d), specials_at_cuts(base, cuts, d), noise, cuts) for d in (-1, 0, -100)] + [(("shard tie", "PSK", world), tie, nt, tcuts)]
    for key, iq, thr, cc in cases:
        bounds = bounds_of(cc, len(iq))
        ref = reference(oracle, key, iq, "PSK", 2, thr, 0.0, 1.5, E.PSK_SPS)
        p = params("PSK", 2, thr, 0.0, 1.5, E.PSK_SPS)
        dev = torch.from_numpy(iq).cuda()
        single = pipe.iq_to_bits(dev, p, want_qad=True, cap_rows=len(iq) // (TOL + 1) + 2)
        assert_result(single, ref, (key, "single"))
        shards = [dev[a:b] for a, b in bounds]
        halos = [None] + [dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a] for a, _ in bounds[1:]]
        res, recs, err = run_sharded(engines, shards, bounds, len(iq), p, halos, timeout=120)
        assert not any(err), err
        for k, (a, b) in enumerate(zip(stitch(res), (ref[1],) + tuple(ref[2]))):
            assert np.array_equal(a, b), (key, bounds, k)
        assert_qad(np.concatenate([r.qad.cpu().numpy() for r in res]), ref[0], (key, bounds))


# ---- segmentation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,full_scale", [(np.int8, False), (np.int16, False), (np.int16, True)])
def test_segment_messages_with_ties(pipe, oracle, dtype, full_scale):
    """the reference compares magnitudes with `>` here: a tie is not above the noise"""
    import torch
    from urh_amd import estimators
    iq, nt = E.tie_segments_capture(dtype, full_scale)
    want = oracle.segment_messages_from_magnitudes(oracle.get_magnitudes(iq), nt)
    merged = oracle.segment_messages_from_magnitudes(oracle.get_magnitudes(iq), float(np.nextafter(np.float32(nt), np.float32(0))))
    assert len(want) == 3 and len(merged) < 3                    # three messages; with the ties above the noise they would merge
    got = estimators.segment_messages_dev(pipe, torch.from_numpy(iq).cuda(), nt)
    assert got == [(int(a), int(b)) for a, b in want], (np.dtype(dtype).name, full_scale, got)
