"""What a batch of captures asks of the library, locked against recorded traces (tests/golden/batch_trace/traces.json), as
tests/test_pipeline_call_trace.py has it for a single pass: for every scenario the ordered names of the urhgpu_* functions called (the
Context's methods included; plain integer arguments -- k, total, policies, capacities, flags -- where they are no addresses), the pipeline's
device and pinned buffers afterwards as {key: elements}, what launch_counts counted, and per capture truncated, n_samples, the noise and
center flags, a hash of bits, pauses and msg_off, and the number of records.  The batch's other GPU tests compare results bit for bit and
count launches; they do not see a buffer that changed its key or its size, a second upload, or a host wait that crept in.  The traces were
recorded with tests/call_trace.py's recorder against the single-module urh_amd/batch.py that the package urh_amd/batch/ replaced
(DESIGN.md 4).  Only the public surface is used -- DevicePipeline's methods, BatchBits, launch_counts --, so the file runs against either.

The scenarios, each on a fresh DevicePipeline (buffer sizes depend on what ran before), captures of 0 to 8193 samples, three to six per
scenario, one of 0 samples and one of 1 among them: iq_to_bits_batch over the input forms (a host list, device tensors, a packed device
tensor without and with gaps, int16), a capture routed through a pass, want_qad; iq_to_bits_batch_auto with noise flags 1, 2 and 0, and
detect_noise_levels; iq_to_bits_batch_center with and without auto_noise, every center flag (1, 0, 2 through a pool of 8 bins, 3 through a
capture whose peaks tie: the second slicing), detect_centers, qad_to_bits_batch; iq_to_bits_batch_records plain, with auto_noise and with a
second slicing; iq_to_bits_batch_psk plain and with every option, costas_demod_batch twice on one pipeline; iq_to_bits_batch_dc (FSK, a
packed device tensor taken whole, PSK, a routed capture) and dc_correct_batch; retry(k) of a truncated capture once per family;
segment_messages_batch, and estimate_batch on one mixed session (seven captures: OOK, ASK and FSK pooled, one given as PSK, one routed, and
the two tiny ones).

`PYTHONPATH=.:oracle python tests/test_batch_call_trace.py` rewrites the fixture from the code as it is -- only from a commit whose calls
are known good."""
import hashlib
import json
import os

import numpy as np
import pytest

import batch_auto_cases
import batch_dc_cases
import batch_estimate_cases
import batch_psk_cases as P
import center_cases as cc
import dc_cases
import noise_cases as nc
from call_trace import recording, trace
from conftest import synth_fsk

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_trace", "traces.json")
DIVISOR = 8
LONG_FROM = 4096
CAP_ROWS = 4                                   # rows per capture of the retry scenarios: every real capture truncates
# the idle rings hold (event, buffer) lists whose content depends on event timing: that the key exists is recorded, not what it holds
RINGS = ("batch_costas_stages", "batch_dc_stages")
# the arguments that are plain integers (k, total, policies, capacities, flags), by position; never an address or a size made from one
INT_ARGS = {
    "urhgpu_ctx_set_tuning": (1, 2), "urhgpu_iq_to_bits_dev": (2,), "urhgpu_iq_to_bits_auto_center_dev": (2, 4), "urhgpu_iq_to_bits_auto_dev": (2, 4, 5, 6),
    "urhgpu_grab_pulse_lens_dev": (2, 5), "urhgpu_ppseq_to_bits_dev": (3,), "urhgpu_msg_records_dev": (2, 5, 7), "urhgpu_outputs_to_host": (2,),
    "urhgpu_batch_plan": (1, 3, 4), "urhgpu_iq_to_bits_batch_dev": (2, 5, 9, 13), "urhgpu_batch_fetch": (2, 6), "urhgpu_batch_noise_dev": (2, 5),
    "urhgpu_iq_to_bits_batch_auto_dev": (2, 5, 9, 13), "urhgpu_batch_noise_fetch": (2,), "urhgpu_batch_center_plan": (1, 2, 3),
    "urhgpu_batch_center_dev": (2, 4, 6, 9, 11, 13, 15), "urhgpu_qad_to_bits_batch_dev": (2, 5, 8, 11, 15),
    "urhgpu_iq_to_bits_batch_center_dev": (2, 5, 7, 8, 11, 15, 18, 20, 22, 24), "urhgpu_batch_center_fetch": (2, 4, 7),
    "urhgpu_batch_msg_records_dev": (2, 4, 7, 10, 12, 16), "urhgpu_batch_records_fetch": (2, 3), "urhgpu_batch_segments_dev": (2, 3, 6, 10, 14),
    "urhgpu_batch_segments_fetch": (2, 6), "urhgpu_batch_demod_dev": (2, 5), "urhgpu_batch_costas_dev": (2, 5),
    "urhgpu_iq_to_bits_batch_psk_dev": (2, 5, 7, 8, 9, 12, 16, 19, 21, 23, 25), "urhgpu_batch_dc_correct_dev": (2, 3, 6)}


def to_dev(pipe, iq):
    import torch
    return torch.from_numpy(np.array(iq)).to(pipe.device)


def with_tiny(real, at=1):
    """the captures with one of 0 samples and one of 1 (the first capture's first sample) put in from position `at`"""
    real = [np.ascontiguousarray(c) for c in real]
    return real[:at] + [real[0][:0].copy(), real[0][:1].copy()] + real[at:]


def packed(caps, gaps=False):
    """(iq_cat, starts) on the host: back to back, or from sample 3 with 5 unused samples behind the last capture"""
    dtype = caps[0].dtype
    return batch_dc_cases.pack(caps, dtype) if gaps else batch_dc_cases.pack(caps, dtype, first=0, behind=0)


def tie_capture():
    """the capture of tests/test_pipeline_call_trace.py whose second and third peak tie (center flag 3 at max_size 7500, noise 0.3)"""
    return synth_fsk(8193, sps=cc.SPS, seed=6, noise=0.05, pause_every=2500, pause_len=700, deviation_hz=20e3)


def wide_capture():
    """a capture whose histogram has 34 bins (center_cases.histogram): more than a pool of 8 holds (center flag 2)"""
    return synth_fsk(3000, sps=cc.SPS, seed=3000, noise=0.05, pause_every=2500, pause_len=700, deviation_hz=20e3)


def sets():
    """name -> (captures, parameters)"""
    flags = dict(batch_auto_cases.flag_captures_f32())
    psk = with_tiny([P.gapped(3000, 2, 1)[0], P.psk_capture(2000, 2, 2)[0]])
    dc = with_tiny([dc_cases.generic(np.float32, 3000), dc_cases.generic(np.float32, 2000, seed=1)])
    return {
        "fsk": (with_tiny([cc.capture(3000, np.float32), cc.capture(2000, np.float32)]), cc.params("FSK", np.float32, write_pos=False)),
        "fsk_i16": (with_tiny([cc.capture(3000, np.int16), cc.capture(2000, np.int16)]), cc.params("FSK", np.int16, write_pos=False)),
        "fsk_long": (with_tiny([cc.capture(3000, np.float32), cc.capture(4097, np.float32)]), cc.params("FSK", np.float32, write_pos=False)),
        "noise": (with_tiny([flags["clean"], flags["gates-all"], flags["inf"]]), nc.params("FSK", 1, write_pos=False)),      # flags 1, 2 and 0
        "quiet": (with_tiny([flags["clean"], flags["gates-all"]]), nc.params("FSK", 1, write_pos=False)),
        "center_auto": (with_tiny([cc.capture(3000, np.float32), flags["gates-all"]]), nc.params("FSK", 1, write_pos=False)),
        "wide": (with_tiny([cc.capture(3000, np.float32), wide_capture()]), cc.params("FSK", np.float32, write_pos=False)),
        "tie": (with_tiny([cc.capture(3000, np.float32), tie_capture()]), cc.params("FSK", np.float32, write_pos=False, noise=0.3)),
        "psk": (psk, P.params(2, 0.2)),
        "dc": (dc, cc.params("FSK", np.float32, write_pos=False)),
        "dc_long": (with_tiny([dc_cases.generic(np.float32, 3000), dc_cases.generic(np.float32, 4097)]), cc.params("FSK", np.float32, write_pos=False)),
        "dc_psk": ([np.ascontiguousarray(c + np.array([0.3, -0.2], np.float32)) for c in psk], P.params(2, 0.2)),
    }


def qad_set():
    """(qad_cat, starts): two two-level signals of 3000 and 2000 samples with one of 0 and one of 1 between them"""
    rng = np.random.default_rng(11)
    real = [(np.repeat(np.where(rng.integers(0, 2, n // 50) == 1, 0.3, -0.3), 50) + 0.02 * rng.standard_normal(n)).astype(np.float32) for n in (3000, 2000)]
    parts = [real[0], real[0][:0], real[0][:1], real[1]]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)


def digest(h):
    return hashlib.sha256(h.bits().tobytes() + b"#" + h.pauses.tobytes() + b"#" + h.msg_off.tobytes()).hexdigest()[:12]


def per_capture(res):
    """[truncated, n_samples, noise flag, center flag, hash, records] per capture; where the reference raises, the exception's name first"""
    out = []
    for k in range(len(res)):
        flags = [None if res.noise_flags is None else res.noise_flags[k], None if res.center_flags is None else res.center_flags[k]]
        try:
            h = res[k]
        except (ValueError, OverflowError) as e:
            out.append([type(e).__name__, None] + flags + [None, None])
            continue
        rec = getattr(h, "records", None)
        out.append([h.truncated, h.n_samples] + flags + [digest(h), None if rec is None else len(rec)])
    return out


def numbers(values):
    return [None if v is None else float(v).hex() for v in values]


def scenario(rec, body, tuning=None):
    """the trace of body(pipe) on a fresh pipeline, with the launches and copies the batch entry points counted"""
    from urh_amd.batch import launch_counts
    from urh_amd.pipeline import DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0, tuning=tuning)
    before = launch_counts(pipe)
    results = body(pipe)
    after = launch_counts(pipe)
    out = trace(rec, pipe, results)
    out["pinned"].update({key: "ring" for key in RINGS if key in pipe._pinned})
    out["launches"] = [after[0] - before[0], after[1] - before[1]]
    return out


def retried(res):
    """the first truncated capture once more, then every capture"""
    cut = res.truncated
    res.retry(cut[0])
    return {"cut": cut, "captures": per_capture(res)}


def loud(call):
    """a call for which the reference may raise (detect_noise_level on a capture that gives an infinity): the values, or the exception's name"""
    try:
        return numbers(call())
    except (ValueError, OverflowError) as e:
        return type(e).__name__


def estimate_session():
    """(captures, modulation per capture): OOK, ASK and FSK pooled, one given as PSK, one of 8193 samples that is routed, the two tiny ones"""
    E = batch_estimate_cases
    ook = E.ook_capture(n_pulses=60)
    assert len(ook) <= 8193
    caps = [ook, ook[:0].copy(), nc.capture(7101, 6000, "ASK", 1, np.float32, 0.01, 0.5), ook[:1].copy(), np.ascontiguousarray(E.sps_capture(50, 7202, 6000)[:2900]),
            P.psk_capture(3000, 2, 5)[0], E.sps_capture(20, 7200, 8193)]
    return caps, ["OOK", None, "ASK", None, None, "PSK", None]


def estimates(res):
    out = []
    for k in range(len(res)):
        try:
            e = res[k]
        except (ValueError, OverflowError) as err:
            e = type(err).__name__
        out.append(e if e is None or isinstance(e, str) else [e["modulation_type"], int(e["bit_length"])] + numbers([e["center"], e["tolerance"], e["noise"]]))
    return out


def scenarios():
    """name -> a function of the recorder that runs the scenario and returns its trace"""
    S = sets()
    out = {}

    def add(name, body, tuning=None):
        out[name] = lambda rec: scenario(rec, body, tuning)

    def batch(method, key, *args, form="host", **options):
        caps, p = S[key]

        def body(pipe):
            given = {"host": lambda: list(caps), "device": lambda: [to_dev(pipe, c) for c in caps],
                     "packed": lambda: (to_dev(pipe, packed(caps)[0]), packed(caps)[1]),
                     "gaps": lambda: (to_dev(pipe, packed(caps, True)[0]), packed(caps, True)[1])}[form]()
            res = getattr(pipe, method)(given, p, *args, **options)
            return retried(res) if options.get("cap_rows") == CAP_ROWS else {"cut": None, "captures": per_capture(res)}
        return body

    add("batch/host_list", batch("iq_to_bits_batch", "fsk"))
    add("batch/device_list", batch("iq_to_bits_batch", "fsk", form="device"))
    add("batch/packed", batch("iq_to_bits_batch", "fsk", form="packed"))
    add("batch/packed_gaps", batch("iq_to_bits_batch", "fsk", form="gaps"))
    add("batch/int16", batch("iq_to_bits_batch", "fsk_i16"))
    add("batch/routed", batch("iq_to_bits_batch", "fsk_long", long_from=LONG_FROM))
    add("batch/want_qad", batch("iq_to_bits_batch", "fsk", want_qad=True))
    add("batch/retry", batch("iq_to_bits_batch", "fsk", cap_rows=CAP_ROWS))

    add("auto/flags", batch("iq_to_bits_batch_auto", "noise"))
    add("auto/retry", batch("iq_to_bits_batch_auto", "noise", cap_rows=CAP_ROWS))
    add("auto/detect_noise_levels", lambda pipe: loud(lambda: pipe.detect_noise_levels(list(S["quiet"][0]))))
    add("auto/detect_noise_levels_raises", lambda pipe: loud(lambda: pipe.detect_noise_levels(list(S["noise"][0]))))

    add("center/auto_noise", batch("iq_to_bits_batch_center", "center_auto"))
    add("center/fixed_noise_tie", batch("iq_to_bits_batch_center", "tie", auto_noise=False, center_max_size=7500))
    add("center/small_pool", batch("iq_to_bits_batch_center", "wide", auto_noise=False), tuning={"auto_center_max_bins": 8})
    add("center/retry", batch("iq_to_bits_batch_center", "tie", auto_noise=False, center_max_size=7500, cap_rows=CAP_ROWS))
    add("center/detect_centers", lambda pipe: numbers(pipe.detect_centers(qad_set())))
    add("center/qad_to_bits_batch", lambda pipe: {"cut": None, "captures": per_capture(pipe.qad_to_bits_batch(qad_set(), S["fsk"][1]))})
    add("center/qad_to_bits_batch_centers", lambda pipe: {"cut": None, "captures": per_capture(pipe.qad_to_bits_batch(qad_set(), S["fsk"][1], centers=[0.01, None, None, -0.02]))})

    add("records/plain", batch("iq_to_bits_batch_records", "fsk", DIVISOR))
    add("records/auto_noise", batch("iq_to_bits_batch_records", "quiet", DIVISOR, auto_noise=True))
    add("records/second_slicing", batch("iq_to_bits_batch_records", "tie", DIVISOR, auto_center=True, center_max_size=7500))
    add("records/retry", batch("iq_to_bits_batch_records", "fsk", DIVISOR, cap_rows=CAP_ROWS))

    add("psk/plain", batch("iq_to_bits_batch_psk", "psk"))
    add("psk/every_option", batch("iq_to_bits_batch_psk", "psk", auto_noise=True, auto_center=True, message_length_divisor=DIVISOR))
    add("psk/retry", batch("iq_to_bits_batch_psk", "psk", cap_rows=CAP_ROWS))

    def costas_twice(pipe):
        caps, p = S["psk"]
        first = pipe.costas_demod_batch(list(caps), p)
        second = pipe.costas_demod_batch(list(caps), p, noise=[0.2, 0.2, 0.2, 0.1])
        return [[int(q.shape[0]), [int(s) for s in starts]] for q, starts in (first, second)]
    add("psk/costas_demod_batch_twice", costas_twice)

    add("dc/fsk_host_list", batch("iq_to_bits_batch_dc", "dc"))
    add("dc/packed_whole", batch("iq_to_bits_batch_dc", "dc", form="gaps"))
    add("dc/psk", batch("iq_to_bits_batch_dc", "dc_psk"))
    add("dc/routed", batch("iq_to_bits_batch_dc", "dc_long", long_from=LONG_FROM))
    add("dc/retry", batch("iq_to_bits_batch_dc", "dc", cap_rows=CAP_ROWS))
    for form in ("host", "device"):
        for want_means in (True, False):
            def correct(pipe, form=form, want_means=want_means):
                caps = S["dc"][0]
                got = pipe.dc_correct_batch(list(caps) if form == "host" else (to_dev(pipe, packed(caps, True)[0]), packed(caps, True)[1]), want_means=want_means)
                return [list(got[0].shape), [int(s) for s in got[1]]] + ([list(got[2].shape), str(got[2].dtype)] if want_means else [])
            add(f"dc/dc_correct_batch_{form}{'_means' if want_means else ''}", correct)

    def segments(pipe):
        cases = {name: (iq, thr) for name, iq, thr in batch_estimate_cases.geometry(np.float32)}
        chosen = [cases[name] for name in ("burst-after-10", "len0-above", "len1-above", "dip9-at30", "gain-low-threshold")]
        got = pipe.segment_messages_batch([iq for iq, _ in chosen], [thr for _, thr in chosen])
        return [np.asarray(g).tolist() for g in got]
    add("estimate/segment_messages_batch", segments)

    def estimate(pipe):
        caps, mods = estimate_session()
        return estimates(pipe.estimate_batch(list(caps), modulation=mods, long_from=8193))
    add("estimate/estimate_batch_mixed", estimate)
    return out


def all_traces():
    with recording(INT_ARGS) as rec:
        return json.loads(json.dumps({name: run(rec) for name, run in scenarios().items()}))


@pytest.fixture(scope="module")
def traces():
    return all_traces()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_scenarios_are_the_recorded_ones(traces, recorded):
    assert sorted(traces) == sorted(recorded)


@pytest.mark.parametrize("part", ["calls", "bufs", "pinned", "launches", "results"])
def test_batches_equal_the_recorded_traces(traces, recorded, part):
    for name in sorted(recorded):
        assert traces[name][part] == recorded[name][part], (name, part)


def names(t):
    return [c.split()[0] for c in t["calls"]]


def flags_of(t, column):
    return [r[column] for r in t["results"]["captures"]]


def test_the_recorded_traces_hold_the_cases(recorded):
    """no GPU needed beyond the module's mark: the grounds the scenarios were chosen for are in the fixture itself"""
    def count(name, fn):
        return names(recorded[name]).count(fn)
    # every family through its own entry point, once; the routed capture through a pass in between
    entry = {"batch/host_list": "urhgpu_iq_to_bits_batch_dev", "auto/flags": "urhgpu_iq_to_bits_batch_auto_dev", "center/auto_noise": "urhgpu_iq_to_bits_batch_center_dev",
             "records/plain": "urhgpu_iq_to_bits_batch_dev", "psk/plain": "urhgpu_iq_to_bits_batch_psk_dev", "dc/fsk_host_list": "urhgpu_iq_to_bits_batch_dev"}
    for name, fn in entry.items():
        called = [c for c in names(recorded[name]) if c.startswith("urhgpu_iq_to_bits")]
        assert called == [fn], (name, called)
    assert count("batch/routed", "urhgpu_iq_to_bits_dev") == 1 and count("dc/routed", "urhgpu_iq_to_bits_dev") == 1
    # the sizes: one capture of 0 samples and one of 1 in every batch
    for name, t in recorded.items():
        if isinstance(t["results"], dict):
            sizes = flags_of(t, 1)
            assert 3 <= len(sizes) <= 6 and max(s for s in sizes if s is not None) <= 8193 and 0 in sizes and 1 in sizes, name
    # the flags
    assert {1, 2, 0} <= set(flags_of(recorded["auto/flags"], 2)) and "OverflowError" in flags_of(recorded["auto/flags"], 0)
    assert {1, 0} <= set(flags_of(recorded["center/auto_noise"], 3)) and 1 in flags_of(recorded["center/auto_noise"], 2)
    assert {1, 0, 3} <= set(flags_of(recorded["center/fixed_noise_tie"], 3)) and flags_of(recorded["center/fixed_noise_tie"], 2) == [None] * 4
    assert 2 in flags_of(recorded["center/small_pool"], 3)
    assert recorded["auto/detect_noise_levels_raises"]["results"] == "OverflowError" and isinstance(recorded["auto/detect_noise_levels"]["results"], list)
    # the second slicing: the walk once more, its buffers under ":again", its records queued and fetched once more
    for name, again in (("center/auto_noise", 0), ("center/fixed_noise_tie", 1), ("center/small_pool", 1), ("records/second_slicing", 1), ("records/plain", 0)):
        assert count(name, "urhgpu_qad_to_bits_batch_dev") == again, name
        assert ("batch:walk_in:again" in recorded[name]["bufs"]) == bool(again) and ("batch_stage:again" in recorded[name]["pinned"]) == bool(again), name
    assert count("records/second_slicing", "urhgpu_batch_msg_records_dev") == 2 and count("records/second_slicing", "urhgpu_batch_records_fetch") == 2
    assert "batch:rec:again" in recorded["records/second_slicing"]["bufs"] and "batch_rec:again" in recorded["records/second_slicing"]["pinned"]
    assert count("records/plain", "urhgpu_batch_msg_records_dev") == 1 and flags_of(recorded["records/plain"], 5)[0] > 0
    # retry: a capture truncated, and run again through the entry point of its family
    for family, fn in (("batch", "urhgpu_iq_to_bits_batch_dev"), ("auto", "urhgpu_iq_to_bits_batch_auto_dev"), ("center", "urhgpu_iq_to_bits_batch_center_dev"),
                       ("records", "urhgpu_iq_to_bits_batch_dev"), ("psk", "urhgpu_iq_to_bits_batch_psk_dev"), ("dc", "urhgpu_iq_to_bits_batch_dev")):
        t = recorded[f"{family}/retry"]
        assert t["results"]["cut"] and count(f"{family}/retry", fn) == 2, family
        assert flags_of(t, 0)[t["results"]["cut"][0]] == 0, family                   # (the retried capture fits now)
    assert count("records/retry", "urhgpu_batch_msg_records_dev") == 2 and count("dc/retry", "urhgpu_batch_dc_correct_dev") == 2
    # PSK and DC: the launches alone, the rings
    assert count("psk/costas_demod_batch_twice", "urhgpu_batch_costas_dev") == 2 and recorded["psk/costas_demod_batch_twice"]["launches"][0] == 2
    assert recorded["psk/costas_demod_batch_twice"]["pinned"]["batch_costas_stages"] == "ring"
    assert count("psk/every_option", "urhgpu_batch_msg_records_dev") >= 1 and "urhgpu_iq_to_bits_batch_psk_dev" in names(recorded["psk/every_option"])
    assert count("dc/psk", "urhgpu_iq_to_bits_batch_psk_dev") == 1 and count("dc/packed_whole", "urhgpu_batch_dc_correct_dev") == 1
    for name in recorded:
        if name.startswith("dc/"):
            assert recorded[name]["pinned"]["batch_dc_stages"] == "ring", name
    for form in ("host", "device"):
        assert recorded[f"dc/dc_correct_batch_{form}"]["launches"][0] == 2 and recorded[f"dc/dc_correct_batch_{form}_means"]["launches"][0] == 2
    assert recorded["dc/dc_correct_batch_device"]["results"][0] != recorded["dc/dc_correct_batch_host"]["results"][0]      # (the gaps stay)
    # the estimate: three groups pooled, two captures alone.  SEVEN captures, one more than every other scenario has at most: three pooled ones
    # that carry messages, one given as PSK, one routed and the two tiny ones are seven roles, and none can stand for another
    t = recorded["estimate/estimate_batch_mixed"]
    assert len(t["results"]) == 7 and t["results"][1] is None and t["results"][3] is None and len(recorded["estimate/segment_messages_batch"]["results"]) == 5
    assert [t["results"][k][0] for k in (0, 2, 4)] == ["ASK", "ASK", "FSK"]           # (OOK is estimated as ASK)
    assert names(t).count("urhgpu_batch_demod_dev") == 2 and names(t).count("urhgpu_batch_segments_dev") == 1 and "estimate:in" in t["bufs"]
    assert recorded["estimate/segment_messages_batch"]["launches"][0] == 3


if __name__ == "__main__":
    first, second = all_traces(), all_traces()
    unstable = sorted(name for name in first if first[name] != second[name])
    assert not unstable, unstable                                # a scenario that is not the same twice is no fixture
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(first, indent=0, sort_keys=True) + "\n")
