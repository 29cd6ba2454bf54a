"""The estimate of a session on the GPU (DevicePipeline.estimate_batch, segment_messages_batch; urh_amd/csrc/batch_estimate.hip;
include/urhgpu.h "a batch of captures: message ranges per capture"): every capture's message ranges and parameters against the recorded
results of the real reference (tests/golden/batch_estimate/) and against the single-capture entry points, with no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import batch_estimate_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def _dev(pipe, a):
    return pipe.torch.from_numpy(np.array(a)).to(pipe.device)              # (a copy: the cases are read-only)


@pytest.mark.parametrize("dtype", bc.GEOMETRY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_segments_equal_the_reference_through_the_three_input_forms(pipe, dtype):
    from urh_amd.estimators import segment_messages_dev
    rec = bc.load_ranges()
    cases = bc.geometry(dtype)
    caps, thr = [iq for _, iq, _ in cases], [t for _, _, t in cases]
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    cat = np.concatenate(caps)
    forms = {"numpy list": caps, "device list": [_dev(pipe, c) for c in caps], "packed numpy": (cat, starts), "packed device": (_dev(pipe, cat), starts)}
    for form, given in forms.items():
        got = pipe.segment_messages_batch(given, thr)
        assert len(got) == len(cases)
        for (name, iq, t), g in zip(cases, got):
            assert g.dtype == np.int64 and np.array_equal(g, rec[f"{np.dtype(dtype).name}/{name}"]), (form, name, g.tolist())
    # and each capture alone: the same ranges from a batch of one and from the single-capture entry point
    for (name, iq, t), g in zip(cases, got):
        alone = pipe.segment_messages_batch([iq], t)[0]
        assert np.array_equal(alone, g), name
        assert np.array_equal(segment_messages_dev(pipe, _dev(pipe, iq), t, as_array=True), g), name


def test_segments_of_many_captures(pipe):
    """300 captures of 0 to 40 samples and one of 20 000: more captures than the scan has threads; one threshold for all"""
    rec = bc.load_ranges()
    caps, thr = bc.many()
    got = pipe.segment_messages_batch(caps, thr)
    for i, g in enumerate(got):
        assert np.array_equal(g, rec[f"many/{i}"]), i


def test_c_abi_writes_nothing_outside_the_regions(pipe):
    """the C ABI on buffers the test owns: regions moved apart with a gap behind each, capacity exactly n / 20 + 1, every buffer filled with a
    sentinel and followed by sentinel words"""
    import torch
    from urh_amd import _lib, batch
    from urh_amd.pipeline import DemodParams
    lib, rec = _lib.load(), bc.load_ranges()
    cases = bc.geometry(np.float32)
    caps = [iq for _, iq, _ in cases]
    k = len(caps)
    lengths = np.array([len(c) for c in caps], np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    caps_of = lengths // 20 + 1
    gap = 3
    region = np.concatenate([[gap], gap + np.cumsum(caps_of + gap)[:-1]]).astype(np.int64)
    cap_seg = int(region[-1] + caps_of[-1] + gap)
    plan, _, _ = batch.batch_plan(lengths, DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False).to_c(np.float32))
    SENT = -0x5A5A5A5A5A5A5A5B
    tail = 8
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(pipe.device)      # noqa: E731
    d_iq, d_start, d_plan, d_region = dev(np.concatenate(caps)), dev(starts), dev(plan), dev(region)
    d_thr = dev(np.array([t for _, _, t in cases], np.float32))
    d_seg = torch.full((2 * cap_seg + tail,), SENT, dtype=torch.int64, device=pipe.device)
    d_out = torch.full((2 * cap_seg + tail,), SENT, dtype=torch.int64, device=pipe.device)
    d_counts = torch.full((k + tail,), SENT, dtype=torch.int64, device=pipe.device)
    d_dir = torch.full((k + 1 + tail,), SENT, dtype=torch.int64, device=pipe.device)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    before = batch.launch_counts(pipe)
    _lib.check(lib.urhgpu_batch_segments_dev(pipe.ctx.handle, C.c_void_p(d_iq.data_ptr()), _lib.DT_F32, int(starts[-1]), C.c_void_p(d_start.data_ptr()),
                                             C.c_void_p(d_plan.data_ptr()), k, C.c_void_p(d_thr.data_ptr()), C.c_void_p(d_region.data_ptr()),
                                             C.c_void_p(d_seg.data_ptr()), cap_seg, C.c_void_p(d_counts.data_ptr()), C.c_void_p(d_dir.data_ptr()),
                                             C.c_void_p(d_out.data_ptr()), cap_seg))
    torch.cuda.synchronize()
    assert tuple(np.subtract(batch.launch_counts(pipe), before)) == (3, 0)
    seg, out, counts, dir_ = (t.cpu().numpy() for t in (d_seg, d_out, d_counts, d_dir))
    want = [rec[f"float32/{name}"] for name, _, _ in cases]
    assert counts[:k].tolist() == [len(w) for w in want] and (counts[k:] == SENT).all()
    assert dir_[:k + 1].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and (dir_[k + 1:] == SENT).all()
    written = np.zeros(2 * cap_seg + tail, bool)
    for c in range(k):
        a = 2 * int(region[c])
        assert np.array_equal(seg[a:a + 2 * len(want[c])].reshape(-1, 2), want[c]), cases[c][0]
        written[a:a + 2 * len(want[c])] = True
    assert (seg[~written] == SENT).all()                     # the gaps, the unused ends of the regions, the words behind the buffer
    m = int(dir_[k])
    assert np.array_equal(out[:2 * m].reshape(-1, 2), np.concatenate(want)) and (out[2 * m:] == SENT).all()
    # a region that does not lie inside the buffer stores nothing and still counts; a refused start is an empty capture
    bad_region = region.copy()
    bad_region[4] = cap_seg                              # (its first pair lies at the buffer's end)
    bad_region[6] = -1
    d_seg.fill_(SENT), d_out.fill_(SENT), d_counts.fill_(SENT)
    _lib.check(lib.urhgpu_batch_segments_dev(pipe.ctx.handle, C.c_void_p(d_iq.data_ptr()), _lib.DT_F32, int(starts[-1]), C.c_void_p(d_start.data_ptr()),
                                             C.c_void_p(d_plan.data_ptr()), k, C.c_void_p(d_thr.data_ptr()), C.c_void_p(dev(bad_region).data_ptr()),
                                             C.c_void_p(d_seg.data_ptr()), cap_seg, C.c_void_p(d_counts.data_ptr()), C.c_void_p(d_dir.data_ptr()),
                                             C.c_void_p(d_out.data_ptr()), cap_seg))
    torch.cuda.synchronize()
    seg, counts = d_seg.cpu().numpy(), d_counts.cpu().numpy()
    assert counts[:k].tolist() == [len(w) for w in want]
    for c in (4, 6):
        a = 2 * int(region[c])
        assert len(want[c]) > 0 and (seg[a:a + 2 * int(caps_of[c])] == SENT).all()
    assert (seg[2 * cap_seg:] == SENT).all()


def _expected(session, name):
    want = bc.load_estimates()[name]
    assert len(want) == len(session["captures"])
    return want


@pytest.mark.parametrize("name", sorted(bc.sessions()))
def test_estimates_equal_the_reference_and_estimate_dev(pipe, name):
    """entry k of estimate_batch == the real reference's AutoInterpretation.estimate of capture k (recorded; no capture is left out) ==
    estimators.estimate_dev of capture k alone; where the reference raises, the entry raises the same exception and the others are handed out"""
    from urh_amd.estimators import estimate_dev
    s = bc.sessions()[name]
    k = len(s["captures"])
    want = _expected(s, name)
    noise, mods = bc.per_capture(s["noise"], k), bc.per_capture(s["modulation"], k)
    got = pipe.estimate_batch(s["captures"], noise=s["noise"], modulation=s["modulation"])
    assert len(got) == k
    left_out = 0
    for i in range(k):
        if isinstance(want[i], str):
            with pytest.raises((ValueError, OverflowError)) as e:
                got[i]
            assert type(e.value).__name__ == want[i], (name, i)
            with pytest.raises(type(e.value)):
                estimate_dev(pipe, _dev(pipe, s["captures"][i]), noise=noise[i], modulation=mods[i])
            continue
        assert bc.same_estimate(got[i], want[i]), (name, i, got[i], want[i])
        alone = estimate_dev(pipe, _dev(pipe, s["captures"][i]), noise=noise[i], modulation=mods[i])
        assert bc.same_estimate(got[i], alone), (name, i, got[i], alone)
    assert left_out == 0


def test_an_entry_does_not_depend_on_its_place(pipe):
    """a capture's entry is the same whether it stands first, last or alone; packed on the device gives what the list gives"""
    s = bc.sessions()["mixed-detect"]
    caps = list(s["captures"])
    base = list(pipe.estimate_batch(caps))
    for i in (0, 4, 5):
        others = [c for j, c in enumerate(caps) if j != i]
        assert bc.same_estimate(pipe.estimate_batch([caps[i]] + others)[0], base[i])
        assert bc.same_estimate(pipe.estimate_batch(others + [caps[i]])[-1], base[i])
        assert bc.same_estimate(pipe.estimate_batch([caps[i]])[0], base[i])
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    packed = list(pipe.estimate_batch((_dev(pipe, np.concatenate(caps)), starts)))
    assert all(bc.same_estimate(a, b) for a, b in zip(packed, base))
    # long captures take their place through estimate_dev
    routed = list(pipe.estimate_batch(caps, long_from=10000))
    assert all(bc.same_estimate(a, b) for a, b in zip(routed, base))


def test_launches_do_not_depend_on_the_number_of_captures(pipe):
    """urhgpu_batch_launches moves by the same amount for 3 and for 300 captures of one message each: for the segmentation alone and for the
    whole estimate (300 messages are one group of batch.MSG_GROUP)"""
    from urh_amd import batch
    one = np.ascontiguousarray(bc.sps_capture(50, 7202, 6000)[:2900])
    assert len(bc.load_ranges()) and len(pipe.segment_messages_batch([one], 0.05)[0]) == 1
    moved = {}
    for k in (3, 300):
        caps = [one] * k
        a = batch.launch_counts(pipe)
        seg = pipe.segment_messages_batch(caps, 0.05)
        b = batch.launch_counts(pipe)
        est = pipe.estimate_batch(caps, noise=None, modulation="FSK")
        c = batch.launch_counts(pipe)
        assert all(len(x) == 1 for x in seg) and all(e is not None and e["bit_length"] == 50 for e in est)
        moved[k] = (tuple(np.subtract(b, a)), tuple(np.subtract(c, b)))
    assert moved[3] == moved[300]
    assert moved[3][0] == (3, 2) and moved[3][1] == (1 + 3 + 1, 1 + 2)      # noise, segmentation, demodulation; the noise blocks, directory, ranges


def test_auto_detect_batch_sets_what_auto_detect_sets(pipe):
    from urh_amd.signal import Signal, auto_detect_batch
    caps = [bc.sessions()["mixed-detect"]["captures"][i] for i in (0, 1, 2, 4)]

    a, b = [Signal(c, pipe=pipe) for c in caps], [Signal(c, pipe=pipe) for c in caps]
    ret = auto_detect_batch(a, detect_modulation=True, detect_noise=True)
    want = [s.auto_detect(detect_modulation=True, detect_noise=True) for s in b]
    assert ret == want and ret == [True, False, True, True]
    for x, y in zip(a, b):
        assert (x.modulation_type, x.samples_per_symbol, x.tolerance) == (y.modulation_type, y.samples_per_symbol, y.tolerance)
        assert float(x.center) == float(y.center) and float(x.noise_threshold) == float(y.noise_threshold)
