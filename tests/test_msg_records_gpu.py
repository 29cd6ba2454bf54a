"""Message records inside a pass, on the GPU (include/urhgpu.h: urhgpu_msg_record; urh_amd/csrc/msg_records.hip): one-shot passes with and
without shipped positions, capture streams (push and push_upload, the captures overwritten as soon as their results are handed out), the
combinations with auto_noise / auto_center, the host-wait counter and the refusal for sharded passes -- against what the REAL reference's
ProtocolAnalyzer.get_protocol_from_signal recorded (tests/golden/msg_records/, tests/golden/messages.json) and, where a pass decides its
own threshold or center, against the numpy model of the record arithmetic (tests/model_msg_records.py) applied to the pass's own outputs.
Equality throughout: bits, pauses, positions, RSSI (== or both NaN), timestamp."""
import dataclasses
import json
import os

import numpy as np
import pytest

import model_msg_records as mm
import msg_record_cases as mc

pytestmark = pytest.mark.gpu


def host_syncs():
    from urh_amd import _lib
    return int(_lib.load().urhgpu_test_records_host_syncs())


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def piped():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0, pipelined=True)


@pytest.fixture(scope="module")
def gold():
    return mc.load()


def to_dev(pipe, iq):
    import torch
    a = np.array(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(pipe.device).view(torch.uint16)
    return torch.from_numpy(a).to(pipe.device)


def one_shot(pp, g, divisor, want_pos, **kw):
    m = g["meta"]
    dev = to_dev(pp, g["iq"])
    res = pp.iq_to_bits(dev, mc.params(m, want_pos), want_qad=True, msg_records=True, message_length_divisor=divisor, **kw)
    return res, dev


# ---- 1. one pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_pos", [True, False], ids=["pos", "no-pos"])
@pytest.mark.parametrize("case,divisor", mc.pairs(), ids=lambda v: str(v))
def test_one_pass_equals_the_reference(pipe, gold, case, divisor, want_pos):
    g = gold[case]
    m = g["meta"]
    one_shot(pipe, g, divisor, want_pos)[0].check_capacity()                 # (scratch of this shape in place)
    before = host_syncs()
    res, dev = one_shot(pipe, g, divisor, want_pos)
    assert host_syncs() == before                                          # queued: no host wait, nothing read back
    msgs = res.message_data(m["sample_rate"], m["timestamp"])
    mc.assert_messages(msgs, g["want"][divisor], (case, divisor, want_pos))
    rec = res.records
    assert rec.dtype.itemsize == 32 and (rec["flag"] == 1).all()
    assert [int(v) for v in rec["first_pos"]] == [int(x.bit_sample_pos[0]) for x in msgs]
    assert [int(v) for v in rec["mid_pos"]] == [int(x.bit_sample_pos[int(len(x.plain_bits) / 2)]) for x in msgs]
    # the pass's own outputs are untouched by the records: flat() is the unpadded digitisation
    plain = g["want"][1] if m["modulation_type"] == "ASK" else g["want"][divisor]
    assert np.array_equal(res.flat()[0], plain["bits"]) and np.array_equal(res.flat()[2], plain["pauses"])
    assert (res.pos_buf is not None) == want_pos


@pytest.mark.parametrize("case,divisor", [("pad", 8), ("m70", 8), ("m1500", 2), ("w9000-float32", 1), ("fsk4", 1), ("u16nan", 1)], ids=lambda v: str(v))
def test_one_pass_on_a_pipelined_context(piped, gold, case, divisor):
    """the records run on the tail stream behind the pass's tail; urhgpu_ctx_join covers them"""
    g = gold[case]
    for want_pos in (True, False):
        res, dev = one_shot(piped, g, divisor, want_pos)
        mc.assert_messages(res.message_data(g["meta"]["sample_rate"], g["meta"]["timestamp"]), g["want"][divisor], (case, want_pos))


def test_get_protocol_equals_the_committed_messages(pipe):
    """the existing golden captures: protocol.get_protocol_from_signal_dev (one pass with records) and the same without shipped positions
    against tests/golden/messages.json; Signal.get_protocol through the records as well"""
    import torch
    from conftest import GOLDEN_DIR, load_golden
    from urh_amd.pipeline import DemodParams
    from urh_amd.protocol import get_protocol_from_signal_dev
    from urh_amd.signal import Signal
    want = json.load(open(os.path.join(GOLDEN_DIR, "messages.json")))
    for key, msgs in want.items():
        name, divisor = key.split("|")
        g = load_golden(name)
        p = DemodParams(g["modulation_type"], g["bits_per_symbol"], g["noise_threshold"], g["center"], g["center_spacing"],
                        g["tolerance"], g["samples_per_symbol"], g["costas_loop_bandwidth"], g["pause_threshold"], True)
        dev = torch.from_numpy(g["iq"]).cuda()
        runs = [get_protocol_from_signal_dev(pipe, dev, p, message_length_divisor=int(divisor)),
                pipe.iq_to_bits_checked(dev, dataclasses.replace(p, write_bit_sample_pos=False), msg_records=True,
                                        message_length_divisor=int(divisor)).message_data()]
        if g["modulation_type"] != "PSK":                                  # (the Signal's PSK first sample: test_signal_shim's subject)
            s = Signal(None, pipe=pipe)
            s.iq = g["iq"]
            for k in ("modulation_type", "bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
                      "costas_loop_bandwidth"):
                setattr(s, k, g[k])
            s.message_length_divisor = int(divisor)
            runs.append(s.get_protocol())
        for got in runs:
            assert len(got) == len(msgs), key
            for a, b in zip(got, msgs):
                assert a.plain_bits_str == b["bits"] and a.pause == b["pause"] and list(a.bit_sample_pos) == b["pos"], key
                assert mc.same_float(a.rssi, b["rssi"]), (key, a.rssi, b["rssi"])
                if b["pos"][0] != 0:            # a message at sample 0 has timestamp 0, which urh's Message replaces by time.time()
                    assert a.timestamp == b["timestamp"], key


def test_records_entry_point_rejects_what_it_cannot_run(pipe, gold):
    import ctypes as C
    import torch
    from urh_amd import _lib
    g = gold["pad"]
    res, dev = one_shot(pipe, g, 8, True)
    lib, cp, o = _lib.load(), mc.params(g["meta"]).to_c(np.float32), res._outputs
    rec = torch.zeros(64 * 32 + 16, dtype=torch.uint8, device=pipe.device)
    args = (pipe.ctx.handle, C.c_void_p(dev.data_ptr()), len(g["iq"]), C.byref(cp), C.byref(o))
    assert lib.urhgpu_msg_records_dev(*args, 0, C.c_void_p(rec.data_ptr()), 64, None) == _lib.ERR_ARG           # divisor
    assert lib.urhgpu_msg_records_dev(*args, 8, C.c_void_p(rec.data_ptr() + 8), 64, None) == _lib.ERR_ARG       # misaligned block
    o2 = _lib.Outputs()
    C.memmove(C.byref(o2), C.byref(o), C.sizeof(_lib.Outputs))
    o2.pos = None
    assert lib.urhgpu_msg_records_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), len(g["iq"]), C.byref(cp), C.byref(o2), 8, C.c_void_p(rec.data_ptr()), 64,
                                      None) == _lib.ERR_ARG                                                     # no positions to read
    assert lib.urhgpu_msg_records_dev(*args, 8, C.c_void_p(rec.data_ptr()), 64, None) == 0
    pipe.ctx.sync()


# ---- 2. capture streams ------------------------------------------------------------------------------------------------------------
def family(gold, prefix):
    names = sorted(n for n in gold if n.startswith(prefix) and n[len(prefix):].isdigit())
    order = names + names[::-1]                                            # every capture twice, sizes going up and down
    return order


@pytest.mark.parametrize("want_pos", [True, False], ids=["pos", "no-pos"])
@pytest.mark.parametrize("route", ["push", "push_upload"])
@pytest.mark.parametrize("prefix,divisor", [("sa", 8), ("sf", 1)])
def test_stream_results_carry_their_records(gold, prefix, divisor, route, want_pos):
    """the captures interleaved through one stream; every capture's device tensor (and pinned source) is overwritten as soon as the result
    that covers it has been handed out -- the records kernel reads the capture later than anything else of its pass, so a result handed
    out before that kernel has finished would show here; no push makes the host wait"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0)
    order = family(gold, prefix)
    m = gold[order[0]]["meta"]
    p = mc.params(m, want_pos)
    st = pipe.stream(max(len(gold[n]["iq"]) for n in order), p, want_qad=True, want_pos=want_pos, dtype=np.dtype(m["dtype"]), msg_records=True,
                     message_length_divisor=divisor)
    host = [torch.from_numpy(np.array(gold[n]["iq"])).pin_memory() for n in order]
    dev = [torch.empty_like(h, device=pipe.device) if route == "push_upload" else h.to(pipe.device) for h in host]
    seen = []

    def keep(r):
        if r is None:
            return
        r.check()
        k = r.seq
        dev[k].fill_(93)                                                    # the capture is the caller's again
        if route == "push_upload":
            host[k].fill_(93)
        g = gold[order[k]]
        mc.assert_messages(r.message_data(m["sample_rate"], m["timestamp"]), g["want"][divisor], (order[k], k, route, want_pos))
        assert (r.pos32 is not None) == want_pos
        seen.append(k)
    before, moved = None, None
    for k in range(len(order)):
        if k == 4:
            before = host_syncs()                                          # (warmed up: every slot has run once)
        keep(st.push(dev[k]) if route == "push" else st.push_upload(host[k], dev[k]))
    moved = host_syncs() - before
    for r in st.flush():
        keep(r)
    st.close()
    assert seen == list(range(len(order)))
    assert moved == 0


def model_messages(iq, flat, mod, sps, bps, divisor, sample_rate, timestamp):
    """what the records of a pass must be, from the pass's OWN flat outputs and the capture (tests/model_msg_records.py)"""
    bits, off, pauses, pos, poff = flat
    rec = mm.records(iq, off, pauses, pos, poff, mod, sps, divisor)
    return rec, mm.padded(bits, off, pauses, pos, poff, rec["n_pad"], sps)


@pytest.mark.parametrize("option", ["auto_noise", "auto_center", "both"])
def test_stream_with_auto_noise_and_auto_center(gold, option):
    """records combined with a threshold / center the pass detects itself: the slicing is then the pass's own, so the records are held
    against the model applied to the result's own outputs -- and the one-shot pass with the same options gives the same"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0)
    name, divisor = ("sa3", 8) if option != "auto_noise" else ("sa5", 8)
    g = gold[name]
    m = g["meta"]
    kw = dict(auto_noise=option in ("auto_noise", "both"), auto_center=option in ("auto_center", "both"))
    p = mc.params(m, True)
    one = pipe.iq_to_bits(to_dev(pipe, g["iq"]), p, want_qad=True, msg_records=True, message_length_divisor=divisor, **kw)
    one_msgs = one.message_data(m["sample_rate"], m["timestamp"])
    st = pipe.stream(len(g["iq"]), p, want_qad=True, want_pos=True, dtype=np.float32, msg_records=True, message_length_divisor=divisor, **kw)
    devs = [to_dev(pipe, g["iq"]) for _ in range(4)]
    results = []
    for d in devs:
        r = st.push(d)
        if r is not None:
            devs[r.seq].fill_(7)
            results.append((r.flat(), r.records.copy(), r.message_data(m["sample_rate"], m["timestamp"])))
    for r in st.flush():
        results.append((r.flat(), r.records.copy(), r.message_data(m["sample_rate"], m["timestamp"])))
    st.close()
    assert len(results) == 4
    for flat, rec, msgs in results:
        want_rec, want_msgs = model_messages(g["iq"], flat, m["modulation_type"], m["samples_per_symbol"], 1, divisor, m["sample_rate"], m["timestamp"])
        assert len(msgs) == len(want_msgs) > 0
        assert np.array_equal(rec["n_pad"], want_rec["n_pad"]) and np.array_equal(rec["first_pos"], want_rec["first_pos"])
        assert np.array_equal(rec["mid_pos"], want_rec["mid_pos"]) and rec["rssi"].tobytes() == want_rec["rssi"].tobytes()
        for a, (bits, pause, pos) in zip(msgs, want_msgs):
            assert list(a.plain_bits) == bits and a.pause == pause and list(a.bit_sample_pos) == pos
        assert [(x.plain_bits_str, x.pause, list(x.bit_sample_pos), x.rssi, x.timestamp) for x in msgs] == \
               [(x.plain_bits_str, x.pause, list(x.bit_sample_pos), x.rssi, x.timestamp) for x in one_msgs]


def test_stream_set_msg_records_only_before_the_first_push(gold):
    import ctypes as C
    from urh_amd import _lib
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0)
    g = gold["sa0"]
    st = pipe.stream(len(g["iq"]), mc.params(g["meta"]), dtype=np.float32, msg_records=True, message_length_divisor=8)
    lib = _lib.load()
    rec, n = C.c_void_p(), C.c_int64(0)
    assert lib.urhgpu_stream_msg_records(st._h, 0, C.byref(rec), C.byref(n)) == _lib.ERR_ARG       # nothing pushed
    st.push(to_dev(pipe, g["iq"]))
    assert lib.urhgpu_stream_set_msg_records(st._h, 1, 8) == _lib.ERR_ARG                          # after the first push
    assert lib.urhgpu_stream_msg_records(st._h, 0, C.byref(rec), C.byref(n)) == _lib.ERR_ARG       # not handed out yet
    (r,) = st.flush()
    mc.assert_messages(r.message_data(g["meta"]["sample_rate"], g["meta"]["timestamp"]), g["want"][8], "sa0")
    st.close()
    plain = pipe.stream(len(g["iq"]), mc.params(g["meta"]), dtype=np.float32)
    plain.push(to_dev(pipe, g["iq"]))
    (r,) = plain.flush()
    with pytest.raises(ValueError):
        r.message_data()                                                    # a stream without records hands out none
    plain.close()


# ---- 3. out of scope -----------------------------------------------------------------------------------------------------------------
def test_sharded_passes_refuse_the_option(gold):
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    sp = ShardedPipeline(None, ThreadComm(ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="sharded"):
        sp.iq_to_bits(None, mc.params(gold["pad"]["meta"]), msg_records=True)
