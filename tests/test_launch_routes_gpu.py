"""Every leaf of the launch sites that choose a kernel instantiation from run-time values (urh_amd/csrc/dispatch.hpp): the sample type, the
modulation, order == 2, write_qad, "noise from the device", the Costas loop order.  Two instantiations that both exist can be swapped at a
site without the code objects showing it, so each site is walked over all the values it accepts and compared with what the suite already
trusts: the oracle for a single capture, the single-capture pass for a capture of a batch, numpy for the casts.

Sites that older tests walk over all their sample types are not repeated here: launch_mag_any (test_gpu_parity::
test_get_magnitudes_equals_oracle), launch_minmax_any (test_auto_interpretation_dropin::test_minmax_equals_reference), launch_chunk_stats
(test_sniffer_gpu::test_chunk_stats_match_numpy), urhgpu_dc_correct_dev (test_dc_correction_gpu::test_sizes_and_forms), the sharded DC
sums and apply (test_shard_dc_gpu::test_sample_types_equal_cuts), urhgpu_batch_dc_correct_dev (test_batch_dc_gpu), launch_sp_mag
(test_shard_estimators_gpu), launch_path_minmax (test_path::test_gpu_paths_equal_reference_and_oracle), launch_convert, all twenty pairs
(test_convert::test_gpu_convert_equals_oracle), the sharded message records (test_shard_msg_records_gpu::
test_synthetic_captures_equal_the_single_gpu_records), launch_seg_finish (test_gpu_parity::test_segment_messages_equals_oracle and
::test_segment_messages_integer_captures), launch_msg_records (test_msg_records_gpu::test_one_pass_equals_the_reference: its fixtures
hold all five types), launch_afp_seam, 5 types x ASK / FSK with the seam value asserted (test_shard_auto_gpu::
test_demodulation_phase_equals_oracle_rows), launch_modulate, float32 / int8 / int16 x ASK / FSK / PSK / OQPSK in a fixed cycle and GFSK
(test_modulate::test_gpu_modulate_equals_goldens_and_oracle, ::test_gpu_gfsk_equals_goldens_and_oracle), and launch_wide_probe
(test_capture_stream::test_integer_stream_switches_to_the_wide_instantiation_and_back: int8 and int16 -- a stream allocates the probe's
result block for signed integer FSK captures only, so no entry point reaches the probe with another type).

Shapes: a single capture has 8192 + 300 samples -- one whole 64-row chunk through the bit-plane kernel and a remainder shorter than a
2048-sample tile through the remainder kernel; a batch has three captures of unequal length below 10 000 samples, one of them empty.
Everything is compared bit for bit: no tolerance."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import batch_psk_cases as P

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.float32]
IDS = [np.dtype(d).name for d in DTYPES]
N_SINGLE = 8192 + 300
BATCH_LENGTHS = (9001, 0, 4097)
TOL, SPS, PAUSE = 5, 20, 8


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def sf():
    from urh_amd import signal_functions
    return signal_functions


def capture(n, dtype, seed):
    """(iq, noise threshold): continuous-phase 2-FSK whose amplitude takes one of four levels per symbol (so that ASK and FSK, orders 2 and 4,
    all have something to slice), two silent stretches, AWGN; integers as conftest.synth_fsk quantises them"""
    rng = np.random.default_rng(seed)
    nsym = n // SPS + 1
    f = np.repeat(np.where(rng.integers(0, 2, nsym) == 1, 20e3, -20e3), SPS)[:n]
    env = np.repeat(0.25 + 0.25 * rng.integers(0, 4, nsym), SPS)[:n]
    ph = np.cumsum(2 * np.pi * f / 1e6)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1).reshape(n, 2) * env[:, None]
    for a in (n // 5, (3 * n) // 5):
        iq[a:a + n // 11] = 0
    iq = iq + 0.01 * rng.standard_normal((n, 2))
    if np.dtype(dtype) == np.float32:
        return iq.astype(np.float32), 0.1
    info = np.iinfo(dtype)
    scale, off = (info.max - info.min) / 2 * 0.7, (info.max + info.min + 1) / 2
    iq = np.clip(np.round(iq * scale + off), info.min, info.max).astype(dtype)
    return iq, (0.0 if np.dtype(dtype).kind == "u" else 0.1 * scale)            # unsigned: the offset dominates |x|, nothing is gated


def params(oracle, iq, noise, mod, bps):
    """center and spacing in the middle of what the oracle demodulates from this capture, so that the slicing has content for every sample type"""
    from urh_amd.pipeline import DemodParams
    center, spacing = 0.0, (1.0 if bps == 1 else 0.3)
    if mod == "ASK" and len(iq) > 2:
        q = oracle.afp_demod(iq, noise, "ASK", 2 ** bps)
        lo, hi = float(q[q > 0].min()) if (q > 0).any() else 0.0, float(q.max())
        center, spacing = float(np.float32((lo + hi) / 2)), float(np.float32(max(hi - lo, 1e-3) / 2 ** bps))
    return DemodParams(mod, bps, noise, center, spacing, TOL, SPS, 0.1, PAUSE, True)


def expected(oracle, iq, p):
    qad = oracle.afp_demod(iq, p.noise_threshold, p.modulation_type, 2 ** p.bits_per_symbol)
    pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    return qad, np.asarray(pp).reshape(-1, 2), oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- a single capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hot_launch_sample_type_modulation_order_and_qad(pipe, oracle, dtype):
    """launch_demod_runs_iq: 5 sample types x ASK / FSK / other x order 2 / 4 x with and without the demodulated signal"""
    iq, noise = capture(N_SINGLE, dtype, seed=1)
    dev = P.to_dev(pipe, iq)
    for mod in ("FSK", "ASK", "QAM"):
        for bps in (1, 2):
            p = params(oracle, iq, noise, mod, bps)
            wq, pp, flat = expected(oracle, iq, p)
            assert len(pp) > 4 or mod == "QAM", (mod, bps)                # (no demodulation branch: the signal stays 0, one row)
            for want_qad in (True, False):
                tag = (np.dtype(dtype).name, mod, bps, want_qad)
                res = pipe.iq_to_bits(dev, p, want_qad=want_qad, cap_rows=len(iq) // (TOL + 1) + 2)
                assert np.array_equal(res.ppseq(), pp), tag
                assert all(np.array_equal(a, b) for a, b in zip(res.flat(), flat)), tag
                if want_qad:
                    assert np.array_equal(u32(res.qad.cpu().numpy()), u32(wq)), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_afp_demod_sample_type_and_modulation(sf, oracle, dtype):
    """launch_afp_demod: 5 sample types x ASK / FSK / other, the chunk through the streaming kernel and the remainder through k_afp_demod"""
    iq, noise = capture(N_SINGLE, dtype, seed=2)
    for mod in ("FSK", "ASK", "QAM"):
        want, got = oracle.afp_demod(iq, noise, mod, 2), sf.afp_demod(iq, noise, mod, 2)
        assert np.array_equal(u32(got), u32(want)), (np.dtype(dtype).name, mod, int((u32(got) != u32(want)).sum()))


@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_costas_sample_type_loop_order_and_route(oracle, dtype, order, route):
    """launch_costas: 5 sample types x loop order 2 / 4 x the host-driven and the device-driven re-speculation (more than two 4096-sample
    chunks, so that the parallel loop runs and not the serial kernel)"""
    from urh_amd import _lib
    from urh_amd import signal_functions as sf
    iq, noise = P.gapped(3 * 4096 + 300, order, seed=3 + order, dtype=dtype)
    ctx = _lib.Context(0)
    if route == "device":
        ctx.set_tuning("costas_dev_rounds", 3)
    want, got = oracle.afp_demod(iq, noise, "PSK", order, 0.1), sf.afp_demod(iq, noise, "PSK", order, 0.1, ctx=ctx)
    assert got[0] == -4.0 and np.array_equal(u32(got[1:]), u32(want[1:])), (np.dtype(dtype).name, order, route)


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16], ids=IDS[:4])
def test_astype_both_directions(pipe, dtype):
    """launch_astype: 4 integer types x to float32 / from float32, against numpy's cast.  The values span each type's WHOLE range --
    negatives for the signed types, values above 127 / 32767 for the unsigned ones, floats with fractions on both sides of zero -- so that
    the signed and the unsigned instantiation of one width give different answers"""
    import torch
    from urh_amd import _lib
    lib, ctx = _lib.load(), pipe.ctx
    rng = np.random.default_rng(5)
    info = np.iinfo(dtype)
    ints = np.concatenate([[info.min, info.max, info.min + 1, info.max - 1], rng.integers(info.min, info.max + 1, 4095)]).astype(dtype)
    assert (ints.astype(np.int64) > np.iinfo(np.int16 if info.bits == 16 else np.int8).max).any() == (info.min == 0) and (ints < 0).any() == (info.min < 0)
    d_src, d_dst = P.to_dev(pipe, ints), torch.empty(len(ints), dtype=torch.float32, device=pipe.device)
    code = {np.int8: _lib.DT_I8, np.uint8: _lib.DT_U8, np.int16: _lib.DT_I16, np.uint16: _lib.DT_U16}[dtype]
    _lib.check(lib.urhgpu_astype_dev(ctx.handle, C.c_void_p(d_src.data_ptr()), code, C.c_void_p(d_dst.data_ptr()), _lib.DT_F32, len(ints)))
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), ints.astype(np.float32))
    floats = rng.uniform(info.min + 0.01, info.max + 0.99, 4099).astype(np.float32)      # inside the type's range: truncation toward zero, no wrap
    floats[:4] = [info.min + 0.5, info.max + 0.5, info.max - 0.5, 0.75]
    floats = np.clip(floats, np.float32(info.min), np.nextafter(np.float32(info.max + 1), np.float32(0)))
    d_f = torch.from_numpy(floats).to(pipe.device)
    d_back = P.to_dev(pipe, np.zeros(len(floats), dtype))
    _lib.check(lib.urhgpu_astype_dev(ctx.handle, C.c_void_p(d_f.data_ptr()), _lib.DT_F32, C.c_void_p(d_back.data_ptr()), code, len(floats)))
    torch.cuda.synchronize()
    back = d_back.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == np.uint16 else d_back.cpu().numpy()
    assert np.array_equal(back, floats.astype(dtype))


# ---- a batch of captures ------------------------------------------------------------------------------------------------------------------
def got_of(h):
    return [np.array(x) for x in (h.ppseq(), h.bits(), h.msg_off, h.pauses, h.bit_sample_pos(), h.pos_offsets())]


def single_pass(pipe, iq, p, **kw):
    one = pipe.iq_to_bits(P.to_dev(pipe, iq), replace(p, write_bit_sample_pos=True), want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2, **kw)
    return one, one.host(pool={})


def batch_equals_the_pass(pipe, res, caps, plist, auto_noise=False, auto_center=False, divisor=None, tag=None):
    """capture k of the batch `res` against iq_to_bits on that capture alone with plist[k] and the same options"""
    assert len(res) == len(caps), tag
    flags = res.noise_flags if auto_noise else [1] * len(caps)
    kept = []
    for i, iq in enumerate(caps):                                # (the pipeline's next passes overwrite nothing of the batch, but its views are copied first)
        if flags[i] == 0 or len(iq) == 0:
            kept.append(None)
            continue
        assert res[i].truncated == 0, (tag, i)
        kept.append((got_of(res[i]), res.qad(i).cpu().numpy(), res[i].n_samples, None if divisor is None else np.array(res[i].records)))
    assert sum(k is not None for k in kept) == sum(len(c) > 0 for c in caps), (tag, flags)
    for i, iq in enumerate(caps):
        if kept[i] is None:
            continue
        got, qad, n_samples, rec = kept[i]
        one, h = single_pass(pipe, iq, plist[i], auto_noise=auto_noise, auto_center=auto_center, msg_records=divisor is not None,
                             message_length_divisor=divisor or 1)
        t = (tag, i, len(iq))
        assert h.n_samples == n_samples, t
        for x, y in zip(got, got_of(h)):
            assert np.array_equal(x, y), t
        assert np.array_equal(u32(qad), u32(one.qad.cpu().numpy()[:len(qad)])), t
        if divisor is not None:
            want = one.records
            assert len(rec) == len(want), t
            for f in ("first_pos", "mid_pos", "n_pad", "flag"):
                assert np.array_equal(rec[f], want[f]), (t, f)
            assert np.array_equal(np.ascontiguousarray(rec["rssi"]).view(np.uint64), np.ascontiguousarray(want["rssi"]).view(np.uint64)), t


def batch_captures(dtype, seed):
    made = [capture(n, dtype, seed + k) for k, n in enumerate(BATCH_LENGTHS)]
    return [iq for iq, _ in made], made[0][1]


VARIANTS = ["plain", "auto_noise", "center", "center+auto_noise", "records"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_walks(pipe, oracle, dtype, variant):
    """launch_batch_bits, launch_batch_noise + launch_batch_bits_dn, launch_batch_demod (noise configured / from the device) +
    launch_batch_bits_qin, urhgpu_batch_msg_records_dev: 5 sample types x ASK / FSK x order 2 / 4 each"""
    caps, noise = batch_captures(dtype, seed=10)
    for mod in ("FSK", "ASK"):
        for bps in (1, 2):
            p = replace(params(oracle, caps[0], noise, mod, bps), write_bit_sample_pos=False)
            tag = (np.dtype(dtype).name, variant, mod, bps)
            kw = dict(want_qad=True, cap_rows="bound")
            if variant == "plain":
                batch_equals_the_pass(pipe, pipe.iq_to_bits_batch(caps, p, **kw), caps, [p] * 3, tag=tag)
            elif variant == "auto_noise":
                batch_equals_the_pass(pipe, pipe.iq_to_bits_batch_auto(caps, p, **kw), caps, [p] * 3, auto_noise=True, tag=tag)
            elif variant == "center":
                batch_equals_the_pass(pipe, pipe.iq_to_bits_batch_center(caps, p, auto_noise=False, **kw), caps, [p] * 3, auto_center=True, tag=tag)
            elif variant == "center+auto_noise":
                batch_equals_the_pass(pipe, pipe.iq_to_bits_batch_center(caps, p, auto_noise=True, **kw), caps, [p] * 3, auto_noise=True, auto_center=True, tag=tag)
            else:
                batch_equals_the_pass(pipe, pipe.iq_to_bits_batch_records(caps, p, message_length_divisor=8, **kw), caps, [p] * 3, divisor=8, tag=tag)


@pytest.mark.parametrize("divisor", [None, 8], ids=["bits", "records"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_with_parameters_per_capture(pipe, oracle, dtype, divisor):
    """launch_each_walk (5 sample types x the ASK and the FSK walk of one batch) and urhgpu_batch_msg_records_each_dev (5 sample types)"""
    caps, noise = batch_captures(dtype, seed=20)
    caps = caps + [caps[0][:3001]]
    plist = [replace(params(oracle, caps[0], noise, mod, bps), write_bit_sample_pos=False) for mod, bps in (("ASK", 1), ("FSK", 2), ("FSK", 1), ("ASK", 2))]
    res = pipe.iq_to_bits_batch_each(caps, plist, message_length_divisor=divisor, want_qad=True, cap_rows="bound")
    batch_equals_the_pass(pipe, res, caps, plist, divisor=divisor, tag=(np.dtype(dtype).name, divisor))


@pytest.mark.parametrize("auto_noise", [False, True], ids=["configured", "device-noise"])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_costas(pipe, dtype, order, auto_noise):
    """launch_batch_costas: 5 sample types x loop order 2 / 4 x threshold configured / from the device"""
    made = [P.gapped(n, order, seed=30 + k, dtype=dtype) for k, n in enumerate(BATCH_LENGTHS)]
    caps, p = [iq for iq, _ in made], P.params(order, made[0][1])
    res = pipe.iq_to_bits_batch_psk(caps, p, auto_noise=auto_noise, want_qad=True, cap_rows="bound")
    batch_equals_the_pass(pipe, res, caps, [p] * 3, auto_noise=auto_noise, tag=(np.dtype(dtype).name, order, auto_noise))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_segments(pipe, dtype):
    """launch_batch_segments: 5 sample types, every capture of the batch against the single-capture entry point"""
    from urh_amd.estimators import segment_messages_dev
    caps, noise = batch_captures(dtype, seed=40)
    thr = noise if noise > 0 else 1.05 * float(np.hypot(*(2.0 ** (8 * caps[0].itemsize - 1),) * 2))       # unsigned: just above the silent stretches' offset
    got = pipe.segment_messages_batch(caps, thr)
    assert len(got) == len(caps) and len(got[1]) == 0
    for i, iq in enumerate(caps):
        if len(iq):
            want = segment_messages_dev(pipe, P.to_dev(pipe, iq), thr, as_array=True)
            assert got[i].dtype == np.int64 and np.array_equal(got[i], want), (np.dtype(dtype).name, i, got[i].tolist(), np.asarray(want).tolist())
    assert noise == 0 or sum(len(g) for g in got) >= 2, [g.tolist() for g in got]      # (signed / float: the threshold separates bursts from silence)


@pytest.fixture(scope="module")
def engines():
    from urh_amd.shard_engine import GpuShardEngine
    return [GpuShardEngine(0) for _ in range(3)]


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sharded_costas_sample_type_and_loop_order(pipe, engines, oracle, dtype, order):
    """launch_costas_shard_spec / launch_costas_shard_resolve: 5 sample types x loop order 2 / 4, three ranks as threads on the one GPU, the
    stitched result against the single-GPU pass and the oracle (tests/test_costas_shard.py's check)"""
    import test_costas_shard as S
    from urh_amd.sharding import shard_bounds
    n = 60_000
    iq, noise = S.psk_capture(n, order, seed=50 + order, dtype=dtype, gaps=((27_000, 28_000),))
    S.check(pipe, engines, iq, S.params(order, noise), shard_bounds(n, 3), oracle)


# ---- what the sites refuse ----------------------------------------------------------------------------------------------------------------
def test_refusals_keep_their_status(pipe):
    """a sample type that does not exist is URHGPU_ERR_DTYPE, and comes before the modulation where both are wrong; a modulation afp_demod
    has no kernel for is URHGPU_ERR_ARG; a cast between two integer types is URHGPU_ERR_DTYPE.  (The batch entry points check both values before
    they reach their launch sites: tests/test_batch_refusals_host.py and the c_abi_guards tests hold those answers.)"""
    import torch
    from urh_amd import _lib
    lib, ctx = _lib.load(), pipe.ctx
    iq = np.zeros((N_SINGLE, 2), np.float32)
    out = np.zeros(N_SINGLE, np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    assert lib.urhgpu_afp_demod(_lib.default_context().handle, vp(iq), 7, N_SINGLE, 0.0, _lib.MOD_FSK, 2, 0.1, 0.0, vp(out)) == _lib.ERR_DTYPE
    assert lib.urhgpu_afp_demod(_lib.default_context().handle, vp(iq), _lib.DT_F32, N_SINGLE, 0.0, 9, 2, 0.1, 0.0, vp(out)) == _lib.ERR_ARG
    assert lib.urhgpu_afp_demod(_lib.default_context().handle, vp(iq), 7, N_SINGLE, 0.0, 9, 2, 0.1, 0.0, vp(out)) == _lib.ERR_DTYPE
    mm = np.zeros(2, np.float32)
    assert lib.urhgpu_minmax(_lib.default_context().handle, vp(out), 7, N_SINGLE, vp(mm)) == _lib.ERR_DTYPE
    a, b = torch.zeros(4096, dtype=torch.float32, device=pipe.device), torch.zeros(4096, dtype=torch.float32, device=pipe.device)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for fn in (lib.urhgpu_convert_dev, lib.urhgpu_astype_dev):
        assert fn(ctx.handle, pa, 7, pb, _lib.DT_F32, 1024) == _lib.ERR_DTYPE
        assert fn(ctx.handle, pa, _lib.DT_F32, pb, 7, 1024) == _lib.ERR_DTYPE
        assert fn(ctx.handle, pa, _lib.DT_F32, pb, _lib.DT_F32, 1024) == _lib.ERR_ARG           # (the entry point: source type == target type)
    assert lib.urhgpu_astype_dev(ctx.handle, pa, _lib.DT_I8, pb, _lib.DT_I16, 1024) == _lib.ERR_DTYPE
    # the other entry points that lead to a dispatched site: a sample type that does not exist
    dh = _lib.default_context().handle
    mags = np.zeros(N_SINGLE, np.float64)
    assert lib.urhgpu_get_magnitudes(dh, vp(iq), 7, N_SINGLE, vp(mags)) == _lib.ERR_DTYPE
    assert lib.urhgpu_afp_demod(dh, vp(iq), 7, N_SINGLE, 0.0, _lib.MOD_PSK, 2, 0.1, 0.0, vp(out)) == _lib.ERR_DTYPE        # (the Costas loop)
    res = torch.zeros(64, dtype=torch.float64, device=pipe.device)
    assert lib.urhgpu_detect_noise_level_dev(ctx.handle, pa, 7, 1024, C.c_void_p(res.data_ptr())) == _lib.ERR_DTYPE
    assert lib.urhgpu_path_minmax_dev(ctx.handle, pa, 7, 0, 1024, 16, pb) == _lib.ERR_DTYPE
    n_seg, n_mrg, amb = C.c_int64(0), C.c_int64(0), C.c_int(0)
    assert lib.urhgpu_message_ranges_dev(ctx.handle, pa, 7, 1024, 0.1, pb, 8, C.byref(n_seg), None, 0, C.byref(n_mrg), C.byref(amb)) == _lib.ERR_DTYPE
    # (urhgpu_dc_correct_dev, urhgpu_shard_dc_sums_dev and urhgpu_chunk_power_stats_dev: test_dc_correction_gpu::test_empty_and_rejected,
    # test_shard_dc_gpu::test_refusals_of_the_entry_points, test_sniffer_gpu::test_chunk_stats_argument_errors)
    assert lib.urhgpu_shard_dc_apply_dev(ctx.handle, pa, 8, 7, (C.c_float * 2)(0.0, 0.0), pb) == _lib.ERR_DTYPE
    # modulate: float32, int8 and int16 only; ASK / FSK / PSK / OQPSK (GFSK has an entry point of its own)
    bits, par, mod_out = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8), np.array([-1.0, 1.0], np.float32), np.zeros((64, 2), np.float32)
    modulate = lambda mod, dtype: lib.urhgpu_modulate(dh, vp(bits), 8, 4, mod, vp(par), 1, 1.0, 1e4, 0.0, 1e6, 0, 0, dtype, vp(mod_out))      # noqa: E731
    assert modulate(_lib.MOD_FSK, _lib.DT_F32) == _lib.OK
    assert modulate(_lib.MOD_FSK, _lib.DT_U8) == _lib.ERR_DTYPE and modulate(_lib.MOD_FSK, _lib.DT_U16) == _lib.ERR_DTYPE
    assert modulate(_lib.MOD_FSK, 7) == _lib.ERR_DTYPE
    assert modulate(9, _lib.DT_F32) == _lib.ERR_UNSUPPORTED and modulate(_lib.MOD_OTHER, _lib.DT_F32) == _lib.ERR_UNSUPPORTED


def test_the_seam_value_is_refused_for_what_has_no_kernel(engines):
    """urhgpu_shard_demod_dev (launch_afp_seam on every rank but the first): ASK and FSK only, URHGPU_ERR_UNSUPPORTED for anything else, and
    URHGPU_ERR_DTYPE for a sample type that does not exist.  (Its ten leaves: test_shard_auto_gpu::test_demodulation_phase_equals_oracle_rows.)"""
    import torch
    from urh_amd import _lib
    from urh_amd.pipeline import DemodParams
    e = engines[0]
    dev = torch.zeros((6400, 2), dtype=torch.float32, device=e.device)
    p = DemodParams("QAM", 1, 0.1, 0.0, 1.0, TOL, SPS, 0.1, PAUSE, False)
    with pytest.raises(_lib.UrhGpuError) as refused:
        e.demod(dev[3200:], dev[3198:3200], 3200, 6400, 1, 2, p)
    assert refused.value.status == _lib.ERR_UNSUPPORTED
    e._pre = None
