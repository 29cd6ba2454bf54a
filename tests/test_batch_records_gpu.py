"""Message records of a batch of captures on the GPU (DevicePipeline.iq_to_bits_batch_records; urh_amd/csrc/batch_records.hip; include/urhgpu.h
"a batch of captures: message records per capture") against what the REAL reference recorded for every session of tests/golden/batch_records/
-- every capture opened alone, with its own detected threshold and center where the variant says so -- and against the single pass on the
capture alone (iq_to_bits(..., msg_records=True)), record for record.  Equality throughout: bits, pauses, positions, RSSI (by bit pattern:
equal, or both NaN), timestamp."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import batch_record_cases as br
import msg_record_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def gold():
    return br.load()


def to_dev(pipe, iq):
    import torch
    a = np.ascontiguousarray(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(pipe.device).view(torch.uint16)
    return torch.from_numpy(a).to(pipe.device)


def same_records(a, b, what):
    """two record arrays field by field, the RSSI by its bit pattern"""
    assert len(a) == len(b), (what, len(a), len(b))
    for f in ("first_pos", "mid_pos", "n_pad", "flag"):
        assert np.array_equal(a[f], b[f]), (what, f)
    assert np.array_equal(np.ascontiguousarray(a["rssi"]).view(np.uint64), np.ascontiguousarray(b["rssi"]).view(np.uint64)), (what, a["rssi"], b["rssi"])


def single_pass(pipe, iq, p, divisor, an, ac):
    """the capture alone through a pass with records: (records, message list maker)"""
    res = pipe.iq_to_bits(to_dev(pipe, iq), p, want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2, auto_noise=an, auto_center=ac, msg_records=True,
                          message_length_divisor=divisor)
    return res.records.copy(), res


def run(pipe, form, s, variant, divisor):
    an, ac = br.VARIANTS[variant]
    caps = [np.ascontiguousarray(c) for c in s["captures"]]
    if form == "numpy":
        given = caps
    elif form == "tensors":
        given = [to_dev(pipe, c) for c in caps]
    else:
        given = (to_dev(pipe, s["iq"]), s["starts"])
    return pipe.iq_to_bits_batch_records(given, br.params(s["meta"]), divisor, auto_noise=an, auto_center=ac, cap_rows="bound")


# ---- 1. every session, every variant, the three input forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", sorted({(n, v) for n, v, _ in br.runs()}), ids=lambda v: str(v))
def test_every_session_equals_the_reference_and_the_single_pass(pipe, gold, name, variant):
    s = gold[name]
    m = s["meta"]
    an, ac = br.VARIANTS[variant]
    p = br.params(m)
    forms = ["numpy", "packed"] + (["tensors"] if m["dtype"] != "uint16" else [])      # (torch does not concatenate uint16 tensors)
    for divisor in m["divisors"]:
        first = None
        for form in forms:
            res = run(pipe, form, s, variant, divisor)
            assert len(res) == len(s["captures"]) and res.truncated == []
            br.assert_session(res.messages(m["sample_rate"], s["timestamps"]), s, variant, divisor, (name, variant, divisor, form))
            recs = [np.array(res[k].records) for k in range(len(res))]
            if first is None:
                first = recs
            for k, (a, b) in enumerate(zip(first, recs)):
                same_records(a, b, (name, form, k))
            if an:
                assert [x == y for x, y in zip(res.noise, s["noise"][variant])] == [True] * len(res)
            if ac:
                assert all((c is None and np.isnan(w)) or c == w for c, w in zip(res.centers, s["center"][variant]))
        # every capture of at least one sample: the single pass on it alone, record for record
        for k, iq in enumerate(s["captures"]):
            if len(iq) == 0:
                assert len(first[k]) == 0
                continue
            rec, alone = single_pass(pipe, iq, p, divisor, an, ac)
            same_records(first[k], rec, (name, variant, divisor, s["names"][k]))
            mc.assert_messages(alone.message_data(m["sample_rate"], s["timestamps"][k]), s["want"][(variant, divisor)][k], (name, "alone", k))


# ---- 2. the families of msg_records.npz as batches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sa+pad", "sf"])
def test_the_reused_families_as_batches(pipe, family):
    cases, meta = br.families()[family]
    p = mc.params(meta, want_pos=False)
    for divisor in sorted(set.intersection(*[set(g["meta"]["divisors"]) for g in cases])):
        res = pipe.iq_to_bits_batch_records([g["iq"] for g in cases], p, divisor, cap_rows="bound")
        for k, g in enumerate(cases):
            assert mc.params(g["meta"], want_pos=False) == p
            mc.assert_messages(res.message_data(k, g["meta"]["sample_rate"], g["meta"]["timestamp"]), g["want"][divisor], (family, divisor, k))


# ---- 3. launches and copies ----------------------------------------------------------------------------------------------------------------
def test_launches_and_copies_do_not_depend_on_the_number_of_captures(pipe, gold):
    """the records add 3 launches and 1 copy to their batch (include/urhgpu.h), whatever the number of captures and of messages -- and as
    many again, whatever the number of tied captures, where centers left to the host make a second slicing"""
    import re
    import os
    from urh_amd import batch
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "urhgpu.h")).read()
    stated = re.search(r"(\d) launches per urhgpu_batch_msg_records_dev and (\d) copy per urhgpu_batch_records_fetch", header)
    added = (int(stated.group(1)), int(stated.group(2)))
    assert added == (3, 1)
    tiny = gold["tiny"]
    p = br.params(tiny["meta"])
    for k in (3, 5000):
        caps = [tiny["captures"][i % 300] for i in range(k)]
        counts = []
        for call in (lambda: pipe.iq_to_bits_batch(caps, p), lambda: pipe.iq_to_bits_batch_records(caps, p)):
            before = batch.launch_counts(pipe)
            res = call()
            after = batch.launch_counts(pipe)
            counts.append((after[0] - before[0], after[1] - before[1]))
        assert (counts[1][0] - counts[0][0], counts[1][1] - counts[0][1]) == added and counts[0] == (3, 2), (k, counts)
        want = tiny["want"][("plain", 1)]
        for i in (0, k // 2, k - 1):
            mc.assert_messages(res.message_data(i, tiny["meta"]["sample_rate"], 0.0), _at_zero(want[i % 300], tiny), ("tiny", k, i))
    # tied captures: the second slicing has its own records call
    import batch_center_cases as B
    import urh_oracle
    pc = B.gain_params("FSK")
    classes = [(iq, B.expected_class(B.reference(urh_oracle, iq, pc, None, True, key=("gain", "FSK", "float32", i + 1)), None))
               for i, iq in enumerate(B.gain_sweep("FSK", np.float32)) if len(iq) == 1033]
    tied, plain = [iq for iq, c in classes if c == "tie"], [iq for iq, c in classes if c in ("ok", "none")]
    assert len(tied) >= 5 and len(plain) >= 3
    for k, ties in ((60, 5), (120, 50)):
        caps = [plain[i % len(plain)] for i in range(k - ties)] + [tied[i % len(tied)] for i in range(ties)]
        counts = []
        for call in (lambda: pipe.iq_to_bits_batch_center(caps, pc), lambda: pipe.iq_to_bits_batch_records(caps, pc, auto_noise=True, auto_center=True)):
            before = batch.launch_counts(pipe)
            res = call()
            after = batch.launch_counts(pipe)
            counts.append((after[0] - before[0], after[1] - before[1]))
        assert sum(f == 3 for f in res.center_flags) == ties
        assert (counts[1][0] - counts[0][0], counts[1][1] - counts[0][1]) == (2 * added[0], 2 * added[1]), (k, ties, counts)


def _at_zero(want, session):
    """a fixture entry with its timestamps moved to a capture recorded at 0.0"""
    m = session["meta"]
    return dict(want, timestamp=np.array([0.0 + int(want["pos"][want["pos_off"][i]]) / m["sample_rate"] for i in range(len(want["pauses"]))]))


# ---- 4. truncation, refusal, routing, noise flags, the second slicing ------------------------------------------------------------------------
def test_truncation_and_retry(pipe, gold):
    from urh_amd import _lib
    s = gold["geom-float32"]
    m = s["meta"]
    res = pipe.iq_to_bits_batch_records(s["captures"], br.params(m), 8, cap_rows=20)
    want = s["want"][("plain", 8)]
    short = [k for k, n in enumerate(s["names"]) if n in ("m70", "r63", "r64", "r65", "r129", "seam", "mid", "pad")]
    assert res.truncated == short
    for k in range(len(res)):
        if k in short:
            assert res[k].truncated & 1 and len(res[k].records) == res[k].n_msg and (res[k].records["flag"] == 0).all() and np.isnan(res[k].records["rssi"]).all()
            with pytest.raises(_lib.UrhGpuError, match="capacity"):
                res.message_data(k, m["sample_rate"], s["timestamps"][k])
        else:
            mc.assert_messages(res.message_data(k, m["sample_rate"], s["timestamps"][k]), want[k], ("fits", k))
    for k in short:
        again = res.retry(k)
        assert res[k] is again and not again.truncated
        mc.assert_messages(res.message_data(k, m["sample_rate"], s["timestamps"][k]), want[k], ("retry", k))
    assert res.truncated == []
    br.assert_session(res.messages(m["sample_rate"], s["timestamps"]), s, "plain", 8, "after the retries")


def raw_records(pipe, iq, starts, plan_lengths, p, divisor, dtype, d_map=None, k_all=None, cap_rec=None, misalign=0, walk_starts=None):
    """urhgpu_iq_to_bits_batch_dev and urhgpu_batch_msg_records_dev on buffers this test owns: (status of the records call, counts, rec_dir,
    records, rec_capture)"""
    import torch
    from urh_amd import _lib, batch
    from urh_amd.protocol import RECORD_DTYPE
    lib = _lib.load()
    k = len(plan_lengths)
    cp = p.to_c(dtype)
    cp.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch.batch_plan(plan_lengths, cp, "bound")
    dev = pipe.device
    d_iq = to_dev(pipe, iq)
    d_start = torch.from_numpy(np.asarray(starts, np.int64)).to(dev)
    d_walk = d_start if walk_starts is None else torch.from_numpy(np.asarray(walk_starts, np.int64)).to(dev)
    d_plan = torch.from_numpy(plan).to(dev)
    work = torch.zeros(max(work_bytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(8 * max(k, 1), dtype=torch.int64, device=dev)
    d_dir = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    blob = torch.zeros(max(blob_cap, 16), dtype=torch.uint8, device=dev)
    pipe.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.urhgpu_iq_to_bits_batch_dev(pipe.ctx.handle, C.c_void_p(d_iq.data_ptr()), len(iq), C.c_void_p(d_walk.data_ptr()), C.c_void_p(d_plan.data_ptr()), k,
                                               C.byref(cp), None, C.c_void_p(work.data_ptr()), work_bytes, C.c_void_p(counts.data_ptr()), C.c_void_p(d_dir.data_ptr()),
                                               C.c_void_p(blob.data_ptr()), blob_cap))
    cap = batch.record_capacity(plan) if cap_rec is None else cap_rec
    rec = torch.full((32 * (cap + 2),), 0xEE, dtype=torch.uint8, device=dev)
    rcap = torch.full((cap + 2,), -7, dtype=torch.int32, device=dev)
    rdir = torch.full((k + 1,), -7, dtype=torch.int64, device=dev)
    dm = None if d_map is None else torch.from_numpy(np.asarray(d_map, np.int64)).to(dev)
    st = lib.urhgpu_batch_msg_records_dev(pipe.ctx.handle, C.c_void_p(d_iq.data_ptr()), len(iq), C.c_void_p(d_start.data_ptr()), len(starts) - 1 if k_all is None else k_all,
                                          C.c_void_p(dm.data_ptr()) if dm is not None else None, C.c_void_p(d_plan.data_ptr()), k, C.byref(cp), None, divisor,
                                          C.c_void_p(work.data_ptr()), work_bytes, C.c_void_p(counts.data_ptr()), C.c_void_p(rdir.data_ptr()),
                                          C.c_void_p(rec.data_ptr() + misalign), cap, C.c_void_p(rcap.data_ptr()))
    torch.cuda.synchronize()
    return st, counts.cpu().numpy().reshape(-1, 8), rdir.cpu().numpy(), rec.cpu().numpy().view(RECORD_DTYPE), rcap.cpu().numpy()


def test_a_refused_capture_leaves_its_neighbours_alone(pipe, gold):
    """a capture whose end lies beyond the buffer: the walk refuses it (truncated bit 3), it has no records, the others have theirs -- the one
    in front of it, whose last window runs over its own end, among them"""
    s = gold["geom-int8"]
    m = s["meta"]
    names = ["pad", "trail", "clip", "at0"]
    idx = [s["names"].index(n) for n in names]
    caps = [s["captures"][i] for i in idx]
    iq = np.concatenate(caps)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    bad = starts.copy()
    bad[-1] += 1
    st, counts, rdir, rec, rcap = raw_records(pipe, iq, bad, np.diff(starts), br.params(m), 8, np.int8)
    assert st == 0 and counts[3, 4] & 8 and counts[3, 1] == 0 and rdir[4] == rdir[3] and not counts[:3, 4].any()
    want = s["want"][("plain", 8)]
    for j in (0, 1, 2):
        w = want[idx[j]]
        r = rec[rdir[j]:rdir[j + 1]]
        assert len(r) == len(w["pauses"]) and (r["flag"] == 1).all() and (rcap[rdir[j]:rdir[j + 1]] == j).all()
        assert np.array_equal(r["rssi"].view(np.uint64), w["rssi"].view(np.uint64)) and r["first_pos"].tolist() == [int(w["pos"][a]) for a in w["pos_off"][:-1]]
    total = int(rdir[-1])
    assert (rec[total:]["flag"] == np.frombuffer(b"\xee" * 4, np.int32)[0]).all() and (rcap[total:] == -7).all()      # nothing behind the used records


def test_routing_by_long_from(pipe, gold):
    """a tiny long_from: the captures at or above it go through passes with records and take their places"""
    s = gold["geom-float32"]
    m = s["meta"]
    res = pipe.iq_to_bits_batch_records(s["captures"], br.params(m), 8, cap_rows="bound", long_from=600)
    lengths = [len(c) for c in s["captures"]]
    assert 0 < sum(n >= 600 for n in lengths) < len(lengths)
    br.assert_session(res.messages(m["sample_rate"], s["timestamps"]), s, "plain", 8, "routed")
    routed = [np.array(res[k].records) for k in range(len(res))]           # (copies: the views belong to the pipeline until its next batch)
    whole = pipe.iq_to_bits_batch_records(s["captures"], br.params(m), 8, cap_rows="bound")
    for k in range(len(res)):
        same_records(routed[k], whole[k].records, ("routed", k))


def test_noise_flags_inside_a_batch(pipe):
    """batch_auto_cases.flag_captures_f32: a capture the reference raises for (noise flag 0) raises where it is handed out, one that is gated
    entirely (flag 2) is sliced as two zeros and its records read the real capture -- each as the single pass gives it"""
    import batch_auto_cases as bac
    import noise_cases as nc
    named = [(n, np.ascontiguousarray(c)) for n, c in bac.flag_captures_f32() if n != "constant"]
    # FSK with one sample per symbol and no tolerance: the two zeros of a flag-2 capture are then two bits, so that it HAS a record (ASK slices
    # a zero as a pause)
    p = replace(nc.params("FSK", 1, write_pos=False), samples_per_symbol=1, tolerance=0, center=-0.1)
    res = pipe.iq_to_bits_batch_records([c for _, c in named], p, 8, auto_noise=True, cap_rows="bound")
    flags = dict(zip([n for n, _ in named], res.noise_flags))
    assert flags["inf"] == 0 and flags["gates-all"] == 2 and flags["clean"] == 1
    for k, (name, iq) in enumerate(named):
        if res.noise_flags[k] == 0:
            with pytest.raises(OverflowError):
                res.message_data(k)
            continue
        rec, alone = single_pass(pipe, iq, p, 8, True, False)
        same_records(res[k].records, rec, name)
        got, want = res.message_data(k, 2e6, 3.5), alone.message_data(2e6, 3.5)
        assert len(got) == len(want) and all(list(a.plain_bits) == list(b.plain_bits) and a.pause == b.pause and list(a.bit_sample_pos) == list(b.bit_sample_pos)
                                             and mc.same_float(a.rssi, b.rssi) and a.timestamp == b.timestamp for a, b in zip(got, want)), name
        if res.noise_flags[k] == 2:
            assert res[k].n_samples == 2 and len(rec) == 1 and rec["flag"][0] == 1 and rec["mid_pos"][0] == 1
            # the window is one sample of the REAL capture, not of the two zeros
            import model_msg_records as mm
            assert rec["rssi"][0] == mm.mean64(mm.magnitudes(iq[1:2]) / mm.norm_of(np.float32)) > 0


def test_the_second_slicing_carries_its_own_records(pipe):
    """a batch with centers left to the host: those captures are sliced again with the settled center and their records are those of the second
    slicing, read from the samples where they lie -- each equal to the single pass on the capture alone"""
    import batch_center_cases as B
    import urh_oracle
    pc = B.gain_params("FSK")
    classes = [(iq, B.expected_class(B.reference(urh_oracle, iq, pc, None, True, key=("gain", "FSK", "float32", i + 1)), None))
               for i, iq in enumerate(B.gain_sweep("FSK", np.float32)) if len(iq) == 1033]
    tied, plain = [iq for iq, c in classes if c == "tie"][:4], [iq for iq, c in classes if c == "ok"][:3]
    caps = [plain[0], tied[0], tied[1], plain[1], tied[2], plain[2], tied[3]]
    res = pipe.iq_to_bits_batch_records(caps, pc, 1, auto_noise=True, auto_center=True, cap_rows="bound")
    assert res.center_flags == [1, 3, 3, 1, 3, 1, 3] and res.truncated == []
    n_msgs = 0
    for k, iq in enumerate(caps):
        rec, alone = single_pass(pipe, iq, pc, 1, True, True)
        assert alone.center == res.centers[k]
        same_records(res[k].records, rec, k)
        n_msgs += len(rec)
        a, b = res.message_data(k, 2e6, 1.0), alone.message_data(2e6, 1.0)
        assert [(list(x.plain_bits), x.pause, list(x.bit_sample_pos), x.timestamp) for x in a] == [(list(x.plain_bits), x.pause, list(x.bit_sample_pos), x.timestamp) for x in b]
    assert n_msgs > 0


# ---- 5. the C ABI with a context -------------------------------------------------------------------------------------------------------------
def test_c_abi_guards(pipe, gold):
    from urh_amd import _lib
    s = gold["geom-int8"]
    m = s["meta"]
    p = br.params(m)
    idx = [s["names"].index(n) for n in ("pad", "trail", "at0")]
    caps = [s["captures"][i] for i in idx]
    iq = np.concatenate(caps)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    lengths = np.diff(starts)
    want = [s["want"][("plain", 8)][i] for i in idx]
    # arguments refused with a context, nothing launched: the buffers keep their sentinels
    for kw, status in ((dict(divisor=0), _lib.ERR_ARG), (dict(divisor=(1 << 30) + 1), _lib.ERR_ARG), (dict(misalign=8), _lib.ERR_ARG), (dict(cap_rec=-1), _lib.ERR_ARG),
                       (dict(k_all=2), _lib.ERR_ARG)):
        divisor = kw.pop("divisor", 8)
        st, _, rdir, rec, rcap = raw_records(pipe, iq, starts, lengths, p, divisor, np.int8, **kw)
        assert st == status and (rdir == -7).all() and (rcap == -7).all(), kw
    # a record capacity smaller than the batch's messages: what fits is stored, nothing behind it is touched
    st, counts, rdir, rec, rcap = raw_records(pipe, iq, starts, lengths, p, 8, np.int8, cap_rec=6)
    total = int(rdir[-1])
    assert st == 0 and total == sum(len(w["pauses"]) for w in want) > 6
    flat_rssi = np.concatenate([w["rssi"] for w in want])
    assert np.array_equal(rec["rssi"][:6].view(np.uint64), flat_rssi[:6].view(np.uint64)) and (rcap[6:] == -7).all()
    assert (rec[6:]["n_pad"] == np.frombuffer(b"\xee" * 4, np.int32)[0]).all()
    # a map: the captures in another order, their samples found through it; an index outside [0, k_all) is a refused capture
    order = [2, 0, 1]
    mapped_iq = np.concatenate([caps[j] for j in order])
    walk_starts = np.concatenate([[0], np.cumsum([len(caps[j]) for j in order])]).astype(np.int64)
    # (the walk runs on the captures in the mapped order; the records read the samples of `iq` through the map)
    both = np.concatenate([mapped_iq, iq])
    off = len(mapped_iq)
    st, counts, rdir, rec, rcap = raw_records(pipe, both, starts + off, [len(caps[j]) for j in order], p, 8, np.int8,
                                              d_map=order, k_all=3, walk_starts=walk_starts)
    assert st == 0
    for j, src in enumerate(order):
        r = rec[rdir[j]:rdir[j + 1]]
        assert (rcap[rdir[j]:rdir[j + 1]] == src).all() and (r["flag"] == 1).all()
        assert np.array_equal(r["rssi"].view(np.uint64), want[src]["rssi"].view(np.uint64)), (j, src)
    st, counts, rdir, rec, rcap = raw_records(pipe, both, starts + off, [len(caps[j]) for j in order], p, 8, np.int8,
                                              d_map=[2, 3, -1], k_all=3, walk_starts=walk_starts)
    assert st == 0 and (rec[rdir[0]:rdir[1]]["flag"] == 1).all()
    assert (rec[rdir[1]:rdir[3]]["flag"] == 0).all() and np.isnan(rec[rdir[1]:rdir[3]]["rssi"]).all() and rdir[3] - rdir[1] > 0
    # the fetch: a count beyond the capacity is refused, none copies nothing
    lib = _lib.load()
    assert lib.urhgpu_batch_records_fetch(pipe.ctx.handle, None, 5, 4, None) == _lib.ERR_CAPACITY
    assert lib.urhgpu_batch_records_fetch(pipe.ctx.handle, None, 0, 4, None) == 0
    assert lib.urhgpu_batch_records_fetch(pipe.ctx.handle, None, 2, 4, None) == _lib.ERR_ARG
