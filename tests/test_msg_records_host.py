"""Message records (include/urhgpu.h: urhgpu_msg_record), the parts that need no GPU: the numpy model of the record arithmetic
(tests/model_msg_records.py) against what the REAL reference recorded (tests/golden/msg_records/), numpy's float64 summation order,
the rewritten padding of urh_amd/protocol.py, and the C boundary of the new entry points.

What the summation test settles: a contiguous float64 np.mean IS walked in pieces of the ufunc buffer size (8192 elements), each piece
pairwise, exactly as urh_amd/csrc/pairwise.hpp states it for float32 -- one pairwise tree over the whole array gives other bits at
thousands of the lengths beyond 8192.  The fixture w9000-float32 (a window of 9000 samples through the real reference) pins the same."""
import array

import numpy as np
import pytest

import model_msg_records as mm
import msg_record_cases as mc


@pytest.fixture(scope="module")
def gold():
    return mc.load()


def test_the_fixtures_hold_the_cases(gold):
    """the grounds the fixtures were built for are really in them (what the reference made of the synthetic captures)"""
    sps_seen = {g["meta"]["samples_per_symbol"] for g in gold.values()}
    assert {1, 7, 8, 9, 15, 16, 127, 128, 129, 136, 257, 300, 9000} <= sps_seen
    assert {g["meta"]["dtype"] for g in gold.values()} == {"int8", "uint8", "int16", "uint16", "float32"}
    assert all(len(g["iq"]) <= 20000 for g in gold.values())
    pad = gold["pad"]["want"]
    ln = {d: np.diff(pad[d]["msg_off"]).tolist() for d in (1, 2, 8)}
    assert ln[1] == [1, 5, 13, 6, 8, 3] and ln[2] == [2, 6, 14, 6, 8, 3] and ln[8] == [8, 8, 13, 8, 8, 3]
    assert pad[1]["pauses"].tolist() == [200, 30, 29, 90, 60, 0] and pad[8]["pauses"].tolist() == [130, 0, 29, 70, 60, 0]
    assert [len(gold[k]["want"][1]["pauses"]) for k in ("none", "one", "m70", "m1500")] == [0, 1, 70, 1500]
    assert np.isnan(gold["u16nan"]["want"][1]["rssi"][0]) and not np.isnan(gold["u16nan"]["want"][1]["rssi"][1])
    assert gold["at0"]["want"][1]["pos"][0] == 0
    clip = gold["clip"]
    assert clip["want"][1]["pos"][clip["want"][1]["pos_off"][1]] + clip["meta"]["samples_per_symbol"] > len(clip["iq"])
    assert gold["fsk4"]["meta"]["bits_per_symbol"] == 2
    # a trailing message (one position more than bits, not two) IS padded when the capture ends in a short pause: from 7 bits to 8
    trail = gold["trail"]["want"]
    assert np.diff(trail[1]["msg_off"]).tolist() == [3, 7] and np.diff(trail[8]["msg_off"]).tolist() == [8, 8]
    assert np.diff(trail[1]["pos_off"]).tolist() == [5, 8] and trail[1]["pauses"].tolist() == [300, 51] and trail[8]["pauses"].tolist() == [250, 41]


@pytest.mark.parametrize("case,divisor", mc.pairs(), ids=lambda v: str(v))
def test_model_equals_the_reference(gold, case, divisor):
    """padding decision, positions, RSSI bit for bit (NaN equals NaN) and timestamp, from the unpadded outputs and the capture"""
    g = gold[case]
    m, plain, want = g["meta"], g["want"][1], g["want"][divisor]
    rec = mm.records(g["iq"], plain["msg_off"], plain["pauses"], plain["pos"], plain["pos_off"], m["modulation_type"], m["samples_per_symbol"], divisor)
    assert len(rec) == len(want["pauses"])
    msgs = mm.padded(plain["bits"], plain["msg_off"], plain["pauses"], plain["pos"], plain["pos_off"], rec["n_pad"], m["samples_per_symbol"])
    off, poff = want["msg_off"], want["pos_off"]
    for i, (bits, pause, pos) in enumerate(msgs):
        assert bits == want["bits"][off[i]:off[i + 1]].tolist() and pause == want["pauses"][i] and pos == want["pos"][poff[i]:poff[i + 1]].tolist(), (case, i)
        assert rec["first_pos"][i] == pos[0] and rec["mid_pos"][i] == pos[int(len(bits) / 2)], (case, i)
        assert mc.same_float(float(rec["rssi"][i]), float(want["rssi"][i])), (case, i, rec["rssi"][i], want["rssi"][i])
        assert m["timestamp"] + int(rec["first_pos"][i]) / m["sample_rate"] == want["timestamp"][i], (case, i)


def test_float64_summation_order_equals_numpy_for_every_length():
    """every window length from 1 to 20 000 on random doubles: the spelled-out pairwise order is np.mean's, bit for bit"""
    rng = np.random.default_rng(5)
    a = rng.random(20000) * np.exp(rng.uniform(-8, 8, 20000))
    bad = [n for n in range(1, 20001) if mm.mean64(a[:n]).tobytes() != np.float64(np.mean(a[:n])).tobytes()]
    assert not bad, bad[:10]
    # ... and ONE pairwise tree over the whole array is not it: the pieces of 8192 show from 8193 on
    whole = [n for n in range(8193, 8300) if mm.pairwise_sum(a[:n]) / np.float64(n) != np.mean(a[:n])]
    assert whole and min(whole) > 8192
    # ... and the order matters at these lengths: plain left-to-right summation differs from it somewhere
    assert any(np.float64(sum(a[:n].tolist()) / n) != np.mean(a[:n]) for n in (129, 300, 8193, 20000))
    assert np.isnan(mm.mean64(a[:0]))


@pytest.mark.parametrize("case,divisor", [p for p in mc.pairs() if p[1] > 1], ids=lambda v: str(v))
def test_rewritten_padding_equals_the_reference(gold, case, divisor):
    """protocol.ensure_message_length_multiple (in place, on the reference-shaped lists) and protocol.apply_padding (on the flat arrays)"""
    from urh_amd import protocol
    g = gold[case]
    sps, plain, want = g["meta"]["samples_per_symbol"], g["want"][1], g["want"][divisor]
    off, poff = plain["msg_off"], plain["pos_off"]
    n_msg = len(plain["pauses"])
    bit_data = [array.array("B", plain["bits"][off[i]:off[i + 1]].tobytes()) for i in range(n_msg)]
    pauses = array.array("L", plain["pauses"].tolist())
    bsp = [array.array("L", plain["pos"][poff[i]:poff[i + 1]].tolist()) for i in range(n_msg)]
    protocol.ensure_message_length_multiple(bit_data, sps, pauses, bsp, divisor)
    woff, wpoff = want["msg_off"], want["pos_off"]
    assert [list(b) for b in bit_data] == [want["bits"][woff[i]:woff[i + 1]].tolist() for i in range(n_msg)]
    assert list(pauses) == want["pauses"].tolist()
    assert [list(q) for q in bsp] == [want["pos"][wpoff[i]:wpoff[i + 1]].tolist() for i in range(n_msg)]
    n_pad = protocol.padding_counts(np.diff(off), plain["pauses"], sps, divisor)
    flat = protocol.apply_padding(plain["bits"], off, plain["pauses"], plain["pos"], poff, n_pad, sps)
    for got, key in zip(flat, ("bits", "msg_off", "pauses", "pos", "pos_off")):
        assert np.array_equal(got, want[key]), (case, key)


def test_rewritten_padding_has_no_per_message_position_patching():
    """a smoke check of the rewrite's shape only: whole-array operations, no indexing of a message's last positions, no IndexError handler
    (that the result is the reference's is test_rewritten_padding_equals_the_reference's subject)"""
    import inspect
    from urh_amd import protocol
    src = inspect.getsource(protocol.ensure_message_length_multiple) + inspect.getsource(protocol.apply_padding) + inspect.getsource(protocol.padding_counts)
    assert "IndexError" not in src and "bit_sample_pos[i][-1]" not in src and "bit_sample_pos[i][-2]" not in src


def test_the_c_boundary_of_the_records():
    """the ctypes prototypes exist, the record is 32 bytes laid out as the numpy dtype, and the calls reject bad arguments before any device work"""
    import ctypes as C
    from urh_amd import _lib, protocol
    lib = _lib.load()
    for name in ("urhgpu_msg_records_dev", "urhgpu_stream_set_msg_records", "urhgpu_stream_msg_records", "urhgpu_test_records_host_syncs"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert C.sizeof(_lib.MsgRecord) == 32 == protocol.RECORD_DTYPE.itemsize == mm.RECORD_DTYPE.itemsize
    for name, _ in _lib.MsgRecord._fields_:
        assert getattr(_lib.MsgRecord, name).offset == protocol.RECORD_DTYPE.fields[name][1] == mm.RECORD_DTYPE.fields[name][1], name
    null = C.c_void_p(None)
    assert lib.urhgpu_msg_records_dev(null, null, 10, None, None, 1, null, 0, null) == _lib.ERR_ARG
    assert lib.urhgpu_stream_set_msg_records(null, 1, 8) == _lib.ERR_ARG
    rec, n = C.c_void_p(), C.c_int64(0)
    assert lib.urhgpu_stream_msg_records(null, 0, C.byref(rec), C.byref(n)) == _lib.ERR_ARG
    assert lib.urhgpu_test_records_host_syncs() >= 0
