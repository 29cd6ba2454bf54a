"""Message records of a batch of captures (include/urhgpu.h "a batch of captures: message records per capture"), the parts that need no GPU:
the numpy model of the directory, the sweep and the clipped windows (tests/model_batch_records.py) against what the REAL reference recorded
for every session (tests/golden/batch_records/), the sweep's three positions against host_bits.positions_from_rows, the condition that makes
the clipping case catch its bug, the C boundary, the refusals of the older entry points, and the code objects' metadata."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_record_cases as br
import model_batch_records as mb
import model_msg_records as mm
import msg_record_cases as mc
import model_noise


@pytest.fixture(scope="module")
def gold():
    return br.load()


def tables_of(oracle, iq, meta, noise=None, center=None):
    """(rows, flat) of one capture opened alone: the oracle's afp_demod -> grab_pulse_lens -> _ppseq_to_bits with the session's parameters
    (noise / center: what the reference detected for it; a threshold that gates everything slices zeros(2), Signal.py:474-484)"""
    noise = meta["noise_threshold"] if noise is None or np.isnan(noise) else float(noise)
    center = meta["center"] if center is None or np.isnan(center) else float(center)
    order = 1 << meta["bits_per_symbol"]
    if noise >= model_noise.max_magnitude(iq.dtype):
        qad = np.zeros(2, np.float32)
    else:
        qad = oracle.afp_demod(iq, noise, meta["modulation_type"], order) if len(iq) else np.zeros(0, np.float32)
    pp = oracle.grab_pulse_lens(qad, center, meta["tolerance"], meta["modulation_type"], meta["samples_per_symbol"], meta["bits_per_symbol"],
                                meta["center_spacing"])
    return pp, oracle.ppseq_to_bits_flat(pp, meta["samples_per_symbol"], meta["bits_per_symbol"], True, meta["pause_threshold"])


def session_tables(oracle, s, variant):
    an, ac = br.VARIANTS[variant]
    return [tables_of(oracle, iq, s["meta"], s["noise"][variant][k] if an else None, s["center"][variant][k] if ac else None)
            for k, iq in enumerate(s["captures"])]


def test_the_fixture_holds_the_cases(gold, oracle):
    """the grounds the sessions were built for are really in them"""
    assert {f"gain-{m}-{d}" for m in ("ASK", "FSK") for d in ("float32", "int8", "uint8", "int16", "uint16")} <= set(gold)
    for name, s in gold.items():
        assert all(len(c) <= 20000 for c in s["captures"]), name
        if name.startswith("gain-"):
            assert s["meta"]["variants"] == list(br.VARIANTS) and s["meta"]["divisors"] == ([1, 8] if "ASK" in name else [1])
            assert not np.isnan(s["noise"]["noise"]).any() and np.isnan(s["noise"]["plain"]).all()
            assert sum(len(w["pauses"]) for w in s["want"][("both", 1)]) >= 3
    size = sum(os.path.getsize(os.path.join(br.GOLDEN, f)) for f in os.listdir(br.GOLDEN))
    assert size <= os.path.getsize(os.path.join(mc.GOLDEN, "msg_records", "msg_records.npz"))
    # the automatic variants change what the reference decodes somewhere (else they would test nothing)
    assert any(len(a["pauses"]) != len(b["pauses"]) or not np.array_equal(a["bits"], b["bits"])
               for n, s in gold.items() if n.startswith("gain-") for v in ("noise", "center") for a, b in zip(s["want"][("plain", 1)], s["want"][(v, 1)]))
    assert gold["fsk4"]["meta"]["bits_per_symbol"] == 2
    assert {s["meta"]["samples_per_symbol"] for n, s in gold.items() if n.startswith("w")} == {1, 7, 8, 9, 127, 128, 129, 257, 9000}
    tiny = gold["tiny"]
    counts = [len(w["pauses"]) for w in tiny["want"][("plain", 1)]]
    assert len(counts) == 300 and min(counts) >= 3 and sum(counts) > 1024 and tiny["meta"]["samples_per_symbol"] == 2
    for dt in ("float32", "int8"):
        s = gold[f"geom-{dt}"]
        want = dict(zip(s["names"], s["want"][("plain", 1)]))
        want8 = dict(zip(s["names"], s["want"][("plain", 8)]))
        assert [len(br.capture_of(s, n)) for n in ("n0", "n1", "n2")] == [0, 1, 2]
        assert len(want["none"]["pauses"]) == 0 and len(br.capture_of(s, "none")) > 100 and len(want["m70"]["pauses"]) == 70
        # a trailing message (one position more than bits) padded from the short pause the capture ends in
        assert np.diff(want["trail"]["pos_off"]).tolist()[-1] == np.diff(want["trail"]["msg_off"]).tolist()[-1] + 1
        assert np.diff(want8["trail"]["msg_off"]).tolist()[-1] == 8 > np.diff(want["trail"]["msg_off"]).tolist()[-1]
        # a message at its capture's sample 0, the capture not first in the buffer and in front of it a window that runs over
        i = s["names"].index("at0")
        assert want["at0"]["pos"][0] == 0 and s["starts"][i] > 0 and s["names"][i - 1] == "clip"
        clip = want["clip"]
        assert clip["pos"][clip["pos_off"][-2]] + s["meta"]["samples_per_symbol"] > len(br.capture_of(s, "clip"))
        assert np.abs(br.capture_of(s, "at0")[:3].astype(np.float64)).sum() > 0
        rows = {n: len(tables_of(oracle, br.capture_of(s, n), s["meta"])[0]) for n in s["names"]}
        assert [rows[n] for n in ("r63", "r64", "r65", "r129")] == [63, 64, 65, 129]
        # the seam: rows 0 .. 63 end with the pause that closes the first message; the second one begins with row 64
        pp = tables_of(oracle, br.capture_of(s, "seam"), s["meta"])[0]
        assert pp[63, 0] == -1 and pp[63, 1] > 8 * s["meta"]["samples_per_symbol"] and pp[64, 0] != -1 and len(want["seam"]["pauses"]) == 2
        # the middle bit of `mid` lies inside row 64, a row of three bits, and is not its first
        pp = tables_of(oracle, br.capture_of(s, "mid"), s["meta"])[0]
        sps = s["meta"]["samples_per_symbol"]
        ts = np.concatenate([[0], np.cumsum(pp[:, 1])])
        mid = int(want["mid"]["pos"][len(want["mid"]["bits"]) // 2])
        assert ts[64] < mid < ts[65] and round(pp[64, 1] / sps) == 3
    assert any(int(a) % 2 for a in gold["geom-int8"]["starts"][1:-1])          # an int8 capture starts at an odd sample index


@pytest.mark.parametrize("name,variant,divisor", br.runs(), ids=lambda v: str(v))
def test_model_equals_the_reference(gold, oracle, name, variant, divisor):
    """directory, sweep and clipped windows against the reference's messages of every capture of the session; the sweep's three positions
    against positions_from_rows"""
    from urh_amd.host_bits import positions_from_rows
    s = gold[name]
    m = s["meta"]
    p = br.params(m)
    tabs = session_tables(oracle, s, variant)
    rec_dir, rec, cap = mb.records(s["iq"], s["starts"], [(pp, f[1], f[2]) for pp, f in tabs], m["modulation_type"], m["samples_per_symbol"],
                                   m["bits_per_symbol"], m["pause_threshold"], divisor)
    want = s["want"][(variant, divisor)]
    assert rec_dir.tolist() == mb.directory([len(w["pauses"]) for w in want]).tolist() and (rec["flag"] == 1).all()
    for k, ((pp, flat), w) in enumerate(zip(tabs, want)):
        r = rec[rec_dir[k]:rec_dir[k + 1]]
        assert (cap[rec_dir[k]:rec_dir[k + 1]] == k).all()
        msgs = mm.padded(flat[0], flat[1], flat[2], flat[3], flat[4], r["n_pad"], m["samples_per_symbol"])
        off, poff = w["msg_off"], w["pos_off"]
        for i, (bits, pause, pos) in enumerate(msgs):
            assert bits == w["bits"][off[i]:off[i + 1]].tolist() and pause == w["pauses"][i] and pos == w["pos"][poff[i]:poff[i + 1]].tolist(), (k, i)
            assert r["first_pos"][i] == pos[0] and r["mid_pos"][i] == pos[int(len(bits) / 2)], (k, i)
            assert mc.same_float(float(r["rssi"][i]), float(w["rssi"][i])), (k, i, r["rssi"][i], w["rssi"][i])
            assert s["timestamps"][k] + int(r["first_pos"][i]) / m["sample_rate"] == w["timestamp"][i], (k, i)
        # the three entries the sweep derives are those of the positions derived on the host
        pos, poff = positions_from_rows(pp[:, 0], pp[:, 1], p)
        assert np.array_equal(pos, flat[3]) and np.array_equal(poff, flat[4])
        swept = mb.sweep(pp, flat[1], flat[2], m["modulation_type"], m["samples_per_symbol"], m["bits_per_symbol"], m["pause_threshold"], divisor)
        assert len(swept) == len(flat[2])
        for i, (first, entry, mid, pad, ok) in enumerate(swept):
            mine = pos[poff[i]:poff[i + 1]]
            ln = int(flat[1][i + 1] - flat[1][i])
            kk = (ln + pad) // 2
            assert ok and first == mine[0] and entry == mine[-2]
            assert mid == (mine[kk] if kk <= len(mine) - 2 else mine[-2] + (kk - (len(mine) - 2)) * m["samples_per_symbol"])


@pytest.mark.parametrize("dt", ["float32", "int8"])
def test_reading_through_into_the_neighbour_changes_an_rssi(gold, oracle, dt):
    """the clipping case can catch its bug: the same model with windows that are not clipped at their capture's end gives another RSSI for
    the last message of `clip` (its neighbour begins with strong samples) -- and for no message whose window lies inside its capture"""
    s = gold[f"geom-{dt}"]
    m = s["meta"]
    tabs = [(pp, f[1], f[2]) for pp, f in session_tables(oracle, s, "plain")]
    args = (m["modulation_type"], m["samples_per_symbol"], m["bits_per_symbol"], m["pause_threshold"], 1)
    rec_dir, good, _ = mb.records(s["iq"], s["starts"], tabs, *args)
    _, bad, _ = mb.records(s["iq"], s["starts"], tabs, *args, clip=False)
    differ = np.nonzero([not mc.same_float(float(a), float(b)) for a, b in zip(good["rssi"], bad["rssi"])])[0]
    k = s["names"].index("clip")
    assert int(rec_dir[k + 1]) - 1 in differ.tolist()
    lengths = np.diff(s["starts"])
    for i in differ.tolist():
        c = int(np.searchsorted(rec_dir, i, side="right")) - 1
        assert good["mid_pos"][i] + m["samples_per_symbol"] > lengths[c]


def test_the_c_boundary_of_the_batch_records():
    """the prototypes exist and the calls reject bad arguments before any device work, in the order the header states"""
    from urh_amd import _lib
    from urh_amd.pipeline import DemodParams
    lib = _lib.load()
    for name in ("urhgpu_batch_msg_records_dev", "urhgpu_batch_records_fetch"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    null = C.c_void_p(None)

    def call(p, divisor=1, d_rec=null, cap_rec=0, dtype=np.float32, k=0, k_all=0, d_map=null, sps=None):
        cp = p.to_c(dtype)
        if sps is not None:
            cp.samples_per_symbol = sps
        return lib.urhgpu_batch_msg_records_dev(null, null, 0, null, k_all, d_map, null, k, C.byref(cp), null, divisor, null, 0, null, null, d_rec, cap_rec, null)
    ask = DemodParams("ASK", 1, 0.1, 0.4, 1.0, 5, 10, 0.1, 8, False)
    assert lib.urhgpu_batch_msg_records_dev(null, null, 0, null, 0, null, null, 0, None, null, 1, null, 0, null, null, null, 0, null) == _lib.ERR_ARG
    for mod in ("PSK", "QAM"):
        assert call(DemodParams(mod, 1, 0.1, 0.0, 1.0, 5, 10, 0.1, 8, False)) == _lib.ERR_UNSUPPORTED
    assert call(DemodParams("FSK", 8, 0.1, 0.0, 1.0, 5, 10, 0.1, 8, False)) == _lib.ERR_UNSUPPORTED
    assert call(ask, sps=0) == _lib.ERR_ARG
    for divisor in (0, -1, (1 << 30) + 1):
        assert call(ask, divisor=divisor) == _lib.ERR_ARG
    assert call(ask, cap_rec=-1) == _lib.ERR_ARG
    assert call(ask, d_rec=C.c_void_p(0x1008), cap_rec=4) == _lib.ERR_ARG           # misaligned records
    assert call(ask, k=2, k_all=3) == _lib.ERR_ARG                                  # without a map the two counts are one
    # everything in order but the context: still refused, and only now
    assert call(ask, divisor=1 << 30) == _lib.ERR_ARG
    assert lib.urhgpu_batch_records_fetch(null, null, 0, 0, null) == _lib.ERR_ARG
    assert lib.urhgpu_batch_records_fetch(null, null, -1, 0, null) == _lib.ERR_ARG


def test_the_older_entry_points_still_refuse_and_name_the_new_one():
    from urh_amd import batch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
    for check, call in ((batch.check_batch_options, batch.iq_to_bits_batch), (batch.check_batch_auto_options, batch.iq_to_bits_batch_auto),
                        (batch.check_batch_center_options, batch.iq_to_bits_batch_center)):
        with pytest.raises(ValueError, match="call iq_to_bits") as e:
            check(p, msg_records=True)
        assert "iq_to_bits_batch_records" in str(e.value) and "call iq_to_bits(" in str(e.value)
        with pytest.raises(ValueError, match="call iq_to_bits"):
            call(None, [], p, msg_records=True)
    # the new one: dc_correction and PSK stay refused, a divisor below 1 is an error, all before a device is touched
    batch.check_batch_records_options(p, 8, dc_correction=False)
    with pytest.raises(ValueError, match="call iq_to_bits"):
        batch.iq_to_bits_batch_records(None, [], p, dc_correction=True)
    with pytest.raises(ValueError, match="CaptureStream"):
        batch.iq_to_bits_batch_records(None, [], DemodParams("PSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False))
    with pytest.raises(ValueError, match="message_length_divisor"):
        batch.iq_to_bits_batch_records(None, [], p, message_length_divisor=0)
    with pytest.raises(TypeError):
        batch.iq_to_bits_batch_records(None, [], p, msg_records=True)
    assert callable(DevicePipeline.iq_to_bits_batch_records)
    from urh_amd import protocol
    assert callable(protocol.get_protocols_from_signals_dev)


def test_the_result_sequence_hands_out_messages():
    """BatchBits.message_data / .messages on results that carry records (host only: a HostBits stand-in)"""
    from urh_amd.batch import BatchBits

    class Stub:
        truncated = 0

        def __init__(self, tag):
            self.tag = tag

        def message_data(self, sample_rate, timestamp):
            return [(self.tag, sample_rate, timestamp)]
    res = BatchBits([Stub("a"), Stub("b")], None, [10, 10])
    assert res.message_data(1, 2e6, 5.0) == [("b", 2e6, 5.0)]
    assert res.messages(2e6, [1.0, 2.0]) == [[("a", 2e6, 1.0)], [("b", 2e6, 2.0)]] and res.messages() == [[("a", 1e6, 0.0)], [("b", 1e6, 0.0)]]
    with pytest.raises(ValueError):
        res.messages(1e6, [0.0])


def test_record_capacity_is_the_plans():
    from urh_amd import batch
    plan = np.array([0, 16, 32, 64, 65, 0, 2, 1, 0], np.int64)
    assert batch.record_capacity(plan) == 33 + 33 + 1 and batch.record_capacity(np.zeros(0, np.int64)) == 0


def _assembly(tmp, src, name, include=None):
    from urh_amd import build
    out = os.path.join(tmp, name + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = ["-I", include] if include else []
    return subprocess.Popen([hipcc, *build.FLAGS, *inc, "--offload-device-only", "-S", src, "-o", out], stderr=subprocess.DEVNULL), out


def test_batch_records_kernels_have_no_spills_and_no_scratch(tmp_path):
    from urh_amd import build
    proc, out = _assembly(str(tmp_path), os.path.join(build.CSRC, "batch_records.hip"), "batch_records")
    assert proc.wait() == 0
    asm = open(out).read()
    kernels = re.findall(r"\.name:\s+(\S*k_batch_\S+)", asm)
    # the directory, the positions, the RSSI for the five sample types
    assert len(kernels) == 7 and sum("k_batch_msg_records" in k for k in kernels) == 5, kernels
    assert sum("k_batch_rec_dir" in k for k in kernels) == 1 and sum("k_batch_rec_pos" in k for k in kernels) == 1
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", asm)]
        assert len(values) == 7 and not any(values), (key, values)
    assert "batch_records.hip" in build.SOURCES


def test_moving_the_summation_into_a_header_changed_no_instruction(tmp_path):
    """msg_records.hip as it is, and with rec_sum.hpp's text put back where it was (inside the file's anonymous namespace), compile to the same
    assembly but for the compilation unit's id"""
    from urh_amd import build
    header = open(os.path.join(build.CSRC, "rec_sum.hpp")).read()
    body = header[header.index("namespace urh {") + len("namespace urh {"):header.rindex("}  // namespace urh")]
    body = "\n".join(line for line in body.split("\n") if "records_norm" not in line)
    assert "rec_window_sum" in body and "py_slice" in body and "rec_n_pad" in body and "struct RecShared" in body and "kRecThreads" in body
    src = open(os.path.join(build.CSRC, "msg_records.hip")).read()
    assert src.count('#include "rec_sum.hpp"\n') == 1 and "rec_window_sum(RecShared" not in src           # (one copy: the header's)
    assert 'rec_sum.hpp' in open(os.path.join(build.CSRC, "batch_records.hip")).read()
    before = src.replace('#include "rec_sum.hpp"\n', "").replace("namespace {\n", "namespace {\n" + body + "\n", 1)
    old = os.path.join(str(tmp_path), "msg_records.hip")
    with open(old, "w") as fh:
        fh.write(before)
    a, out_a = _assembly(str(tmp_path), old, "before", include=build.CSRC)
    b, out_b = _assembly(str(tmp_path), os.path.join(build.CSRC, "msg_records.hip"), "after")
    assert a.wait() == 0 and b.wait() == 0

    def text(path):
        return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(path).read())
    assert text(out_a) == text(out_b)
