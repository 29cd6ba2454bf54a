"""DevicePipeline.iq_to_bits_batch_each (urh_amd/batch/each.py; urh_amd/csrc/batch_each.hip; include/urhgpu.h "a batch of captures:
parameters per capture") against the oracle and against iq_to_bits on each capture alone: capture k of a batch comes back with what
params[k] gives for that capture alone, whatever lies beside it in the buffer and whatever the neighbours' parameters are.  Equality
throughout (np.array_equal, floats by their bit patterns); the exactness tests run with cap_rows="bound" and assert that nothing was
truncated."""
import ctypes as C
import os
import re
from dataclasses import replace

import numpy as np
import pytest

from conftest import ROOT, synth_fsk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def dp(mod="FSK", bps=1, noise=0.0, tol=5, sps=100, pt=8, center=None, spacing=None):
    from urh_amd.pipeline import DemodParams
    center = (0.0 if mod == "FSK" else 0.4) if center is None else center
    spacing = (1.0 if bps == 1 else (0.3 if mod == "FSK" else 0.2)) if spacing is None else spacing
    return DemodParams(mod, bps, noise, center, spacing, tol, sps, 0.1, pt, False)


def to_dev(pipe, iq):
    import torch
    a = np.ascontiguousarray(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(pipe.device).view(torch.uint16)
    return torch.from_numpy(a).to(pipe.device)


def expected(oracle, iq, p):
    """tests/test_batch_gpu.py::expected: the capture alone through the oracle with ITS parameters"""
    qad = oracle.afp_demod(iq, p.noise_threshold, p.modulation_type, 2 ** p.bits_per_symbol)
    pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    return qad, np.asarray(pp).reshape(-1, 2), oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)


def same(h, want, qad=None, tag=None):
    wq, pp, flat = want
    assert h.truncated == 0 and h.rows_needed == len(pp), (tag, h.truncated, h.rows_needed, len(pp))
    assert np.array_equal(h.ppseq(), pp), tag
    assert np.array_equal(h.bits(), flat[0]) and np.array_equal(h.msg_off, flat[1]) and np.array_equal(h.pauses, flat[2]), tag
    assert np.array_equal(h.bit_sample_pos(), flat[3]) and np.array_equal(h.pos_offsets(), flat[4]), tag
    for a, b in zip(h.flat(), flat):
        assert np.array_equal(a, b), tag
    if qad is not None:
        assert np.array_equal(qad.cpu().numpy().view(np.uint32), wq.view(np.uint32)), tag


def run_exact(pipe, oracle, caps, params, want_qad=True, **kw):
    res = pipe.iq_to_bits_batch_each(caps, params, want_qad=want_qad, cap_rows="bound", **kw)
    assert len(res) == len(caps) and res.truncated == [] and res.params == list(params)
    for i, (iq, p) in enumerate(zip(caps, params)):
        assert res[i].n_samples == len(iq) and res[i].seq == i and res[i].params == p
        same(res[i], expected(oracle, iq, p), res.qad(i) if want_qad else None, (i, len(iq), p))
    return res


def ask_capture(n, sps, bps, seed, pause_every=0, pause_len=0):
    """a tone whose envelope steps through 2 ** bps levels every sps samples, with silent gaps"""
    iq = synth_fsk(n, sps=sps, seed=seed, noise=0.02, pause_every=pause_every, pause_len=pause_len)
    env = np.repeat(np.random.default_rng(seed).integers(0, 2 ** bps, n // sps + 1), sps)[:n] / (2 ** bps - 1)
    return (iq * (0.05 + 0.95 * env)[:, None]).astype(np.float32)


def cycle_params(k):
    """ASK / FSK x bps {1, 2, 3} x sps {8, 10, 100} x tolerance {0, 5, 70} x pause_threshold {0, 8} x noise {0, 0.1}: strides that are
    coprime with the counts, and a different center in every capture"""
    out = []
    for i in range(k):
        mod = ("ASK", "FSK")[i % 2]
        bps, sps, tol, pt, noise = (1, 2, 3)[(i // 2) % 3], (8, 10, 100)[(i // 3) % 3], (0, 5, 70)[(i // 5) % 3], (0, 8)[(i // 7) % 2], (0.0, 0.1)[(i // 4) % 2]
        center = (0.35 + 0.003 * i) if mod == "ASK" else (-0.02 + 0.0017 * i)
        out.append(dp(mod, bps, noise, tol, sps, pt, center))
    return out


# ---- 1. the mixed batch ---------------------------------------------------------------------------------------------------------------------
def test_a_mixed_batch_in_shuffled_order(pipe, oracle):
    from urh_amd.batch import batch_step
    S = batch_step()
    lengths = [0, 1, 2, 3]
    for tol in (5, 70):
        lengths += [tol - 1, tol, tol + 1]
    lengths += [S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 12_289, 70_001]
    order = np.random.default_rng(1).permutation(len(lengths))
    params = cycle_params(len(lengths))
    assert len({(p.modulation_type, p.center) for p in params}) == len(params)
    caps = []
    for j, i in enumerate(order):
        p, n = params[j], lengths[i]
        if p.modulation_type == "ASK":
            caps.append(ask_capture(n, p.samples_per_symbol, p.bits_per_symbol, int(i), 400, 130))
        else:
            caps.append(synth_fsk(n, sps=p.samples_per_symbol, seed=int(i), noise=0.05, pause_every=400, pause_len=130))
    run_exact(pipe, oracle, caps, params)


def test_the_same_samples_twice_side_by_side(pipe, oracle):
    x = ask_capture(9001, 10, 1, 3, 700, 160) + synth_fsk(9001, sps=10, seed=4, noise=0.0) * np.float32(0.01)
    for a, b in ((dp("ASK", 1, 0.05, 5, 10), dp("FSK", 1, 0.05, 5, 10)), (dp("FSK", 1, 0.05, 5, 10), dp("FSK", 3, 0.05, 5, 10, spacing=0.05)),
                 (dp("ASK", 3, 0.05, 2, 10, spacing=0.1), dp("ASK", 1, 0.05, 2, 10))):
        res = run_exact(pipe, oracle, [x, x], [a, b])
        assert not np.array_equal(res[0].ppseq(), res[1].ppseq())


# ---- 2. neighbours with extreme differences, on buffers this test owns -------------------------------------------------------------------------
def raw_each(pipe, caps, params, gap=48, auto_noise=False):
    """urhgpu_iq_to_bits_batch_each_dev on buffers this test owns, the regions of the work buffer `gap` bytes apart and everything filled with
    0xEE first: (HostBits per capture, the work buffer's bytes, plan, region sizes)"""
    import torch
    from urh_amd import _lib, batch
    from urh_amd.host_bits import HostBits
    from urh_amd.batch.staging import write_noise_blocks
    lib = _lib.load()
    k = len(caps)
    lengths = np.array([len(c) for c in caps], dtype=np.int64)
    table, thr = batch.each_table(params)
    plan, work_bytes, blob_cap = batch.batch_plan_each(lengths, table, "bound")
    sizes = np.diff(np.concatenate([plan[:k], [work_bytes]]))
    plan[:k] += gap * (1 + np.arange(k))                    # (gap is a multiple of 16)
    work_bytes += gap * (k + 1)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    blocks = np.zeros(8 * k, np.int64)
    write_noise_blocks(blocks.ctypes.data, [p.noise_threshold for p in params])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(pipe.device)      # noqa: E731
    d_iq, d_start, d_plan = dev(np.concatenate(caps)), dev(starts), dev(plan)
    d_each, d_thr, d_noise = dev(table.view(np.uint8)), dev(thr if len(thr) else np.zeros(1, np.float32)), dev(blocks)
    work = torch.full((work_bytes,), 0xEE, dtype=torch.uint8, device=pipe.device)
    counts = torch.zeros(8 * k, dtype=torch.int64, device=pipe.device)
    d_dir = torch.zeros(k + 1, dtype=torch.int64, device=pipe.device)
    blob = torch.zeros(blob_cap, dtype=torch.uint8, device=pipe.device)
    qad = torch.zeros(int(starts[-1]), dtype=torch.float32, device=pipe.device)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    _lib.check(lib.urhgpu_iq_to_bits_batch_each_dev(pipe.ctx.handle, p(d_iq), int(starts[-1]), _lib.DT_F32, p(d_start), p(d_plan), k,
                                                    p(d_each), p(d_thr), len(thr), int((table["mod"] == _lib.MOD_ASK).sum()), int(auto_noise), p(qad), p(work),
                                                    work_bytes, p(counts), p(d_dir), p(blob), blob_cap, p(d_noise)))
    torch.cuda.synchronize()
    offs, h_blob = d_dir.cpu().numpy(), blob.cpu().numpy()
    items = []
    for j in range(k):
        h = HostBits.from_blob(h_blob.ctypes.data + int(offs[j]), params[j], seq=j, n_samples=int(lengths[j]))
        h._keep = h_blob
        items.append(h)
    return items, work.cpu().numpy(), plan, sizes, qad.cpu().numpy(), starts


def test_neighbours_with_extreme_differences_stay_inside_their_regions(pipe, oracle):
    wide, narrow = dp("FSK", 1, 0.05, 5, 100), dp("FSK", 3, 0.05, 0, 8, spacing=0.05)
    caps = [synth_fsk(8001, sps=100, seed=1, pause_every=3000, pause_len=900), synth_fsk(8001, sps=8, seed=2, noise=0.2, pause_every=900, pause_len=200),
            synth_fsk(7003, sps=100, seed=3, pause_every=2500, pause_len=1000)]
    params = [wide, narrow, wide]
    gap = 48
    items, work, plan, sizes, qad, starts = raw_each(pipe, caps, params, gap)
    for j, (iq, p) in enumerate(zip(caps, params)):
        want = expected(oracle, iq, p)
        same(items[j], want, None, j)
        assert np.array_equal(qad[starts[j]:starts[j + 1]].view(np.uint32), want[0].view(np.uint32))
    # every region is laid out from ITS tolerance, samples per symbol and bits per symbol (include/urhgpu.h: rows, a byte per bit, offsets, pauses)
    up = lambda x: (x + 15) & ~15                            # noqa: E731
    for j, (iq, p) in enumerate(zip(caps, params)):
        rows = len(iq) // (p.tolerance + 1) + 2
        bits = (len(iq) // p.samples_per_symbol + rows // 2 + 2) * p.bits_per_symbol
        assert sizes[j] == up(8 * rows) + up(bits) + up(8 * (rows // 2 + 2)) + up(8 * (rows // 2 + 1)), j
    assert sizes[1] > 4 * sizes[0]
    used = np.zeros(len(work), bool)
    for j in range(3):
        used[plan[j]:plan[j] + sizes[j]] = True
    assert (~used).sum() == gap * 4 and (work[~used] == 0xEE).all()
    assert (work[used] != 0xEE).any()
    # ... and through the method, beside each other in one upload
    run_exact(pipe, oracle, caps, params)


def test_the_ask_short_pause_rule_takes_the_captures_own_sps(pipe, oracle):
    """a gap of 19 samples (+ tolerance bookkeeping aside: tolerance 0) is a short pause at 20 samples per symbol and an ordinary one at 19"""
    def with_gap(g):
        iq = synth_fsk(4000, sps=20, seed=9, noise=0.0)      # a constant envelope above the center: one state but for the gap
        iq[1000:1000 + g] = 0
        return iq
    caps, params = [], []
    for sps in (19, 20, 21):
        for g in (sps - 1, sps):
            caps.append(with_gap(g))
            params.append(dp("ASK", 1, 0.1, 0, sps, 8, center=0.3))
    res = run_exact(pipe, oracle, caps, params)
    for k, (iq, p) in enumerate(zip(caps, params)):
        states = res[k].ppseq()[:, 0].tolist()
        g = int((iq[1000:1100] == 0).all(axis=1).sum())
        assert (-1 in states) == (g >= p.samples_per_symbol), (k, g, p.samples_per_symbol, states)
    # the same gap, two answers: 19 samples are short for sps 20 and not for sps 19
    assert -1 in res[1].ppseq()[:, 0] and -1 not in res[2].ppseq()[:, 0] and len(caps[1]) == len(caps[2])
    assert int((caps[1][1000:1100] == 0).all(axis=1).sum()) == int((caps[2][1000:1100] == 0).all(axis=1).sum()) == 19


# ---- 3. edge values ------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_samples_and_both_orders_in_one_launch(pipe, oracle):
    import edge_inputs as ei
    caps, params = [], []
    for mod in ("FSK", "ASK"):
        for order, variant in ((2, 0), (4, 1), (2, 2), (4, 0)):
            iq, noise, _ = ei.sprinkled(mod, variant, order, n=8192 + 1032)
            center, spacing = ei.slicing(mod, np.float32, order)
            caps.append(iq)
            params.append(dp(mod, order.bit_length() - 1, noise, 5, ei.SPS, 8, center, spacing))
    assert any(not np.isfinite(c).all() for c in caps)
    res = pipe.iq_to_bits_batch_each(caps, params, want_qad=True, cap_rows="bound")
    assert res.truncated == []
    for k, (iq, p) in enumerate(zip(caps, params)):
        wq, pp, flat = expected(oracle, iq, p)
        assert ei.same_bits(res.qad(k).cpu().numpy(), wq).all(), k       # (the same bit pattern, or a NaN on both sides: tests/test_batch_edges_gpu.py)
        assert np.array_equal(res[k].ppseq(), pp) and all(np.array_equal(a, b) for a, b in zip(res[k].flat(), flat)), k


@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_a_demodulated_value_exactly_on_a_threshold(pipe, oracle, mod):
    iq = ask_capture(3001, 10, 2, 5, 700, 100) if mod == "ASK" else synth_fsk(3001, sps=10, seed=5, noise=0.05, pause_every=700, pause_len=100)
    noise = 0.05
    qad = oracle.afp_demod(iq, noise, mod, 2)
    sentinel = 0.0 if mod == "ASK" else -4.0
    live = np.nonzero(qad != sentinel)[0]
    q0 = qad[live[len(live) // 2]]
    caps, params = [], []
    for bps, spacing in ((1, 1.0), (2, 0.0625), (2, 0.125)):
        # order 2: the threshold IS the center; order 4: center and center +- spacing (powers of two: exact in float32 where q0 - spacing is)
        for center in ((float(q0),) if bps == 1 else (float(q0), float(np.float32(q0) + np.float32(spacing)))):
            p = dp(mod, bps, noise, 1, 10, 8, center, spacing)
            from urh_amd.signal_functions import get_center_thresholds
            thr = np.asarray(get_center_thresholds(p.center, p.center_spacing, 2 ** bps), dtype=np.float32)
            if q0 in thr:
                caps.append(iq)
                params.append(p)
    assert len(params) >= 3 and {p.bits_per_symbol for p in params} == {1, 2}
    run_exact(pipe, oracle, caps, params)


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.uint8, np.uint16])
def test_sample_types(pipe, oracle, dtype):
    scale = float(np.iinfo(dtype).max - np.iinfo(dtype).min) / 2
    caps, params = [], []
    for i, n in enumerate((1, 3, 777, 5, 2049, 4095, 64, 1290)):
        mod = ("FSK", "ASK")[i % 2]
        sps, bps, tol = (20, 10, 8)[i % 3], (1, 2)[(i // 2) % 2], (5, 0, 70)[i % 3]
        caps.append(synth_fsk(n, sps=sps, seed=n, noise=0.1, pause_every=500, pause_len=90, dtype=dtype))
        params.append(dp(mod, bps, 0.2 * scale, tol, sps, (8, 0)[i % 2], center=0.0 if mod == "FSK" else 0.3 + 0.01 * i))
    run_exact(pipe, oracle, caps, params)


# ---- 4. automatic noise thresholds -------------------------------------------------------------------------------------------------------------
def test_auto_noise_per_capture(pipe):
    import batch_auto_cases as bac
    named = [(n, np.ascontiguousarray(c)) for n, c in bac.flag_captures_f32()]
    params = [dp(("FSK", "ASK")[i % 2], 1 + i % 2, 0.0, (0, 5)[i % 2], (1, 10, 50)[i % 3], 8, center=-0.1 if i % 2 == 0 else 0.2) for i in range(len(named))]
    res = pipe.iq_to_bits_batch_each([c for _, c in named], params, auto_noise=True, want_qad=True, cap_rows="bound")
    flags = dict(zip([n for n, _ in named], res.noise_flags))
    # (one NaN sample makes one chunk's mean a NaN, which detect_noise_level's minimum passes over: that capture is handed out)
    assert flags["inf"] == 0 and flags["gates-all"] == 2 and flags["clean"] == 1
    import edge_inputs as ei
    for k, (name, iq) in enumerate(named):
        if res.noise_flags[k] == 0:
            with pytest.raises((OverflowError, ValueError)):
                res[k]
            continue
        # (the pass ships its positions, which a batch derives from the pulse table: write_bit_sample_pos, or flat() holds none to compare)
        alone = pipe.iq_to_bits(to_dev(pipe, iq), replace(params[k], write_bit_sample_pos=True), want_qad=True,
                                cap_rows=len(iq) // (params[k].tolerance + 1) + 2, auto_noise=True)
        assert alone.noise_flag == res.noise_flags[k] and float(alone._noise) == res.noise[k], name
        h = res[k]
        assert h.truncated == 0 and np.array_equal(h.ppseq(), alone.ppseq()), name
        for a, b in zip(h.flat(), alone.flat()):
            assert np.array_equal(a, b), name
        assert ei.same_bits(res.qad(k).cpu().numpy(), alone.qad.cpu().numpy()).all(), name     # (the same bit pattern, or a NaN on both sides)
        if name != "one-nan":
            assert np.array_equal(res.qad(k).cpu().numpy().view(np.uint32), alone.qad.cpu().numpy().view(np.uint32)), name
        if name == "gates-all":
            assert h.n_samples == 2 and res.qad(k).cpu().numpy().tolist() == [0.0, 0.0]


# ---- 5. records ------------------------------------------------------------------------------------------------------------------------------------
def same_records(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in ("first_pos", "mid_pos", "n_pad", "flag"):
        assert np.array_equal(a[f], b[f]), (what, f)
    assert np.array_equal(np.ascontiguousarray(a["rssi"]).view(np.uint64), np.ascontiguousarray(b["rssi"]).view(np.uint64)), (what, a["rssi"], b["rssi"])


@pytest.mark.parametrize("divisor", [1, 8])
def test_records_per_capture(pipe, divisor):
    caps, params = [], []
    for i in range(8):
        mod = ("ASK", "FSK")[i % 2]
        sps, bps = (100, 10, 8, 20)[i % 4], (1, 1, 2, 3)[i % 4]
        n = 9001 + 37 * i
        caps.append(ask_capture(n, sps, bps, i, 2500, 1200) if mod == "ASK" else synth_fsk(n, sps=sps, seed=i, noise=0.03, pause_every=2500, pause_len=1200))
        params.append(dp(mod, bps, 0.1, (5, 1)[i % 2], sps, 8, center=0.3 + 0.01 * i if mod == "ASK" else 0.001 * i))
    # a capture that ENDS inside its last message's middle symbol: the RSSI window is clipped at its own end, the next capture lies directly behind
    tail = synth_fsk(170, sps=100, seed=77, noise=0.01)      # two bits: the middle one's symbol is [101, 201)
    caps.insert(3, tail)
    params.insert(3, dp("FSK", 1, 0.1, 1, 100, 8))
    res = pipe.iq_to_bits_batch_each(caps, params, message_length_divisor=divisor, cap_rows="bound")
    assert res.truncated == []
    padded = {"ASK": 0, "FSK": 0}
    recs = [np.array(res[k].records) for k in range(len(caps))]
    msgs = [res.message_data(k, 2e6, 1.5) for k in range(len(caps))]
    for k, (iq, p) in enumerate(zip(caps, params)):
        alone = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2, msg_records=True, message_length_divisor=divisor)
        rec = alone.records.copy()
        same_records(recs[k], rec, (k, p))
        assert len(rec) > 0 and (rec["flag"] == 1).all(), k
        padded[p.modulation_type] += int((rec["n_pad"] > 0).sum())
        want = alone.message_data(2e6, 1.5)
        assert len(msgs[k]) == len(want) and all(list(a.plain_bits) == list(b.plain_bits) and a.pause == b.pause and a.timestamp == b.timestamp
                                                 and list(a.bit_sample_pos) == list(b.bit_sample_pos) for a, b in zip(msgs[k], want)), k
    assert padded["FSK"] == 0 and (padded["ASK"] > 0) == (divisor == 8)
    # the clipped window: the middle bit's symbol ends beyond the capture
    r = recs[3][-1]
    assert r["mid_pos"] + 100 > len(tail) > r["mid_pos"]


# ---- 6. the other routes -----------------------------------------------------------------------------------------------------------------------
def test_a_uniform_list_gives_the_blobs_of_the_batch_with_one_parameter_set(pipe):
    for p in (dp("FSK", 2, 0.1, 5, 10), dp("ASK", 1, 0.05, 0, 20, center=0.3)):
        caps = [synth_fsk(n, sps=p.samples_per_symbol, seed=n, noise=0.05, pause_every=400, pause_len=130) for n in (0, 1, 5, 777, 12_289, 64, 3001)]
        one = pipe.iq_to_bits_batch(caps, p, cap_rows="bound")
        total = sum(one[k].blob_bytes for k in range(len(caps)))
        want = bytes(one[0]._keep[0].numpy()[:total])
        each = pipe.iq_to_bits_batch_each(caps, [p] * len(caps), cap_rows="bound")
        assert sum(each[k].blob_bytes for k in range(len(caps))) == total and total > 128 * len(caps)
        assert bytes(each[0]._keep[0].numpy()[:total]) == want
        assert bytes(pipe.iq_to_bits_batch_each(caps, p, cap_rows="bound")[0]._keep[0].numpy()[:total]) == want        # a single DemodParams is broadcast


def test_input_forms_dc_corrected_input_and_a_long_capture(pipe, oracle):
    params = cycle_params(6)
    caps = [ask_capture(n, p.samples_per_symbol, p.bits_per_symbol, n, 400, 130) if p.modulation_type == "ASK"
            else synth_fsk(n, sps=p.samples_per_symbol, seed=n, noise=0.05, pause_every=400, pause_len=130) for n, p in zip((3001, 64, 25_001, 777, 0, 5000), params)]
    cat = np.concatenate(caps)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])])
    for given in (caps, [to_dev(pipe, c) for c in caps], (to_dev(pipe, cat), starts), (cat, starts)):
        res = pipe.iq_to_bits_batch_each(given, params, want_qad=True, cap_rows="bound")
        for k, (iq, p) in enumerate(zip(caps, params)):
            same(res[k], expected(oracle, iq, p), res.qad(k), k)
    # the long one goes through a pass with ITS parameters
    routed = pipe.iq_to_bits_batch_each(caps, params, want_qad=True, cap_rows="bound", long_from=20_000)
    for k, (iq, p) in enumerate(zip(caps, params)):
        wq, pp, flat = expected(oracle, iq, p)
        assert np.array_equal(routed[k].ppseq(), pp) and all(np.array_equal(a, b) for a, b in zip(routed[k].flat(), flat)), k
        assert np.array_equal(routed.qad(k).cpu().numpy().view(np.uint32), wq.view(np.uint32)), k
    # what dc_correct_batch returns is the third input form
    shifted = [c + np.float32(0.05) for c in caps]
    d_cat, d_starts = pipe.dc_correct_batch(shifted)
    corrected = d_cat.cpu().numpy()
    res = pipe.iq_to_bits_batch_each((d_cat, d_starts), params, want_qad=True, cap_rows="bound")
    for k, p in enumerate(params):
        same(res[k], expected(oracle, np.ascontiguousarray(corrected[d_starts[k]:d_starts[k + 1]]), p), res.qad(k), ("dc", k))


def test_overflow_and_retry(pipe, oracle):
    rng = np.random.default_rng(0)
    noisy = (0.3 * rng.standard_normal((9001, 2))).astype(np.float32)           # far more rows than four per symbol
    caps = [synth_fsk(3001, sps=10, seed=1), noisy, synth_fsk(2001, sps=100, seed=2)]
    params = [dp("FSK", 1, 0.0, 5, 10), dp("FSK", 2, 0.0, 0, 100), dp("ASK", 1, 0.0, 5, 100)]
    res = pipe.iq_to_bits_batch_each(caps, params, want_qad=True)
    assert res.truncated == [1] and res[1].truncated & 1
    again = res.retry(1)
    same(again, expected(oracle, noisy, params[1]), res.qad(1), "retry")
    assert res.truncated == [] and again.params == params[1]
    for k in (0, 2):
        same(res[k], expected(oracle, caps[k], params[k]), res.qad(k), k)


# ---- 7. launches and copies ------------------------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_captures_or_parameter_sets(pipe):
    """the stated budget: one walk per modulation present (at most two), scan, pack; auto_noise one more; records three more and one copy"""
    from urh_amd import batch
    header = open(os.path.join(ROOT, "include", "urhgpu.h")).read()
    assert re.search(r"ONE walk per modulation present \(at most two", header)
    base = [synth_fsk(600 + 7 * i, sps=10, seed=i, noise=0.05, pause_every=200, pause_len=110) for i in range(10)]

    def moved(call):
        before = batch.launch_counts(pipe)
        call()
        after = batch.launch_counts(pipe)
        return after[0] - before[0], after[1] - before[1]
    seen = {}
    for k, distinct in ((3, 3), (300, 1), (300, 2), (300, 300)):
        caps = [base[i % 10] for i in range(k)]
        # the modulations present held equal: ASK at the even places, FSK at the odd ones, in every set
        params = [dp(("ASK", "FSK")[i % 2], 1 + (i % distinct) % 3, 0.05, (i % distinct) % 7, 8 + (i % distinct) % 90, 8,
                     center=(0.3 if i % 2 == 0 else 0.0) + 0.0001 * (i % distinct)) for i in range(k)]
        n_sets = len({(p.bits_per_symbol, p.tolerance, p.samples_per_symbol, p.center) for p in params})
        assert n_sets >= min(distinct, 2) and (distinct < 300 or n_sets >= 150)
        seen[(k, distinct)] = (moved(lambda: pipe.iq_to_bits_batch_each(caps, params)), moved(lambda: pipe.iq_to_bits_batch_each(caps, params, auto_noise=True)),
                               moved(lambda: pipe.iq_to_bits_batch_each(caps, params, message_length_divisor=1)),
                               moved(lambda: pipe.iq_to_bits_batch_each(caps, params, auto_noise=True, message_length_divisor=8)))
    for key, got in seen.items():
        assert got == ((4, 2), (5, 3), (7, 3), (8, 4)), (key, got)
    one_mod = [dp("FSK", 1 + i % 3, 0.05, i % 7, 8 + i, 8) for i in range(30)]
    assert moved(lambda: pipe.iq_to_bits_batch_each([base[i % 10] for i in range(30)], one_mod)) == (3, 2)
    # the copies are those of iq_to_bits_batch_records
    p = dp("FSK", 1, 0.05, 5, 10)
    caps = [base[i % 10] for i in range(30)]
    assert moved(lambda: pipe.iq_to_bits_batch_records(caps, p))[1] == moved(lambda: pipe.iq_to_bits_batch_each(caps, [p] * 30, message_length_divisor=1))[1]


# ---- 8. the session routes built on the batch --------------------------------------------------------------------------------------------------
def same_messages(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for a, b in zip(got, want):
        assert list(a.plain_bits) == list(b.plain_bits) and a.pause == b.pause and a.timestamp == b.timestamp, what
        assert list(a.bit_sample_pos) == list(b.bit_sample_pos), what
        assert np.float64(a.rssi).view(np.uint64) == np.float64(b.rssi).view(np.uint64), (what, a.rssi, b.rssi)
        assert (a.samples_per_symbol, a.bits_per_symbol) == (b.samples_per_symbol, b.bits_per_symbol), what


def session():
    caps, params = [], []
    for i in range(6):
        mod = ("ASK", "FSK")[i % 2]
        sps, bps = (100, 10, 20)[i % 3], (1, 2)[i % 2]
        n = 8001 + 53 * i
        caps.append(ask_capture(n, sps, bps, 40 + i, 2500, 1200) if mod == "ASK" else synth_fsk(n, sps=sps, seed=40 + i, noise=0.03, pause_every=2500, pause_len=1200))
        params.append(dp(mod, bps, 0.1, (5, 1)[i % 2], sps, 8, center=0.3 + 0.01 * i if mod == "ASK" else 0.001 * i))
    return caps, params


@pytest.mark.parametrize("dc", [False, True])
def test_protocols_of_a_session_with_a_parameter_set_per_capture(pipe, dc):
    from urh_amd.protocol import get_protocols_from_signals_dev
    caps, params = session()
    caps.append(synth_fsk(5000, sps=100, seed=3, noise=0.02))            # a PSK entry is split off and keeps its place
    params.append(dp("PSK", 1, 0.05, 5, 100))
    stamps = [0.5 * k for k in range(len(caps))]
    got = get_protocols_from_signals_dev(pipe, caps, params, 8, 2e6, stamps, dc_correction=dc)
    assert len(got) == len(caps)
    for k, (iq, p) in enumerate(zip(caps, params)):
        alone = pipe.iq_to_bits(to_dev(pipe, iq), replace(p, write_bit_sample_pos=True), want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2,
                                msg_records=True, message_length_divisor=8, dc_correction=dc)
        want = alone.message_data(2e6, stamps[k])
        assert len(want) > 0 or p.modulation_type == "PSK"
        same_messages(got[k], want, (k, dc))
    with pytest.raises(ValueError, match="one DemodParams per capture"):
        get_protocols_from_signals_dev(pipe, caps, params[:-1])
    with pytest.raises(ValueError, match="iq_to_bits_batch_center"):
        get_protocols_from_signals_dev(pipe, caps, params, auto_center=True)


def test_get_protocols_batch_hands_every_signal_its_own_protocol(pipe):
    from urh_amd.signal import Signal, get_protocols_batch
    caps, params = session()

    def signals():
        out = []
        for k, (iq, p) in enumerate(zip(caps, params)):
            s = Signal(iq, modulation=p.modulation_type, sample_rate=1e6 * (1 + k % 2), timestamp=0.25 * k, pipe=pipe)
            s.bits_per_symbol, s.noise_threshold, s.center, s.center_spacing = p.bits_per_symbol, p.noise_threshold, p.center, p.center_spacing
            s.tolerance, s.samples_per_symbol, s.pause_threshold = p.tolerance, p.samples_per_symbol, p.pause_threshold
            s.message_length_divisor = (1, 8)[k % 2 == 0]
            out.append(s)
        out[3].noise_threshold = 2.0                                      # not below max_magnitude: Signal.qad is zeros(2)
        out.append(Signal(synth_fsk(3000, sps=100, seed=9, dtype=np.int8), modulation="FSK", pipe=pipe))       # another sample type: alone
        return out
    got = get_protocols_batch(signals())
    want = [s.get_protocol() for s in signals()]
    assert len(got) == len(want) == 7 and sum(len(w) for w in want) > 6
    for k, (a, b) in enumerate(zip(got, want)):
        same_messages(a, b, k)
