"""What a single-GPU pass asks of the library, locked against recorded traces (tests/golden/pipeline_trace/traces.json): for every scenario
the ordered names of the urhgpu_* functions called (the Context's methods included; plain integer flags where they are no addresses), the
pipeline's device and pinned buffers afterwards as {key: elements}, the host counts and the noise / center flags.  The other tests compare
results bit for bit; they do not see a host wait, a second launch, or a buffer that changed its size or its name -- as
tests/test_shard_call_trace.py has it for the sharded orchestration.  The traces were recorded with tests/call_trace.py's recorder against the
pipeline.py / shard_engine.py whose repeated blocks the shared helpers replaced.

The scenarios: a one-shot pass and a CaptureStream (four pushes and the flush) -- plain, without the demodulated signal, auto_center with
every flag (1, 0, 2 through a pool of 8 bins, 3 through a capture whose peaks tie), auto_noise with flags 1 and 2, both together, DC
correction --, each also with message records, shipped positions or not; then a pipelined context (one slot twice, two slots), qad_to_bits,
iq_to_bits_checked on a capture that needs its second pass (a frequency that alternates every sample: a pulse-table row per sample),
Signal.get_protocol twice and one GpuShardEngine pass of a single rank with host results.  Captures of 806 to 8193 samples.

`PYTHONPATH=.:oracle python tests/test_pipeline_call_trace.py` rewrites the fixture from the code as it is -- only from a commit whose calls
are known good."""
import dataclasses
import json
import os

import numpy as np
import pytest

import center_cases as cc
import dc_cases
import msg_record_cases as mc
import noise_cases as nc
from call_trace import recording, trace
from conftest import synth_fsk

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_trace", "traces.json")
DIVISOR = 8
# the arguments that are plain integers (flags, lengths, capacities), by position; never an address or a size made from one
INT_ARGS = {"urhgpu_ctx_set_pipelined": (1,), "urhgpu_ctx_set_tuning": (1, 2), "urhgpu_iq_to_bits_dev": (2,), "urhgpu_iq_to_bits_auto_center_dev": (2, 4),
            "urhgpu_iq_to_bits_auto_dev": (2, 4, 5, 6), "urhgpu_grab_pulse_lens_dev": (2, 5), "urhgpu_ppseq_to_bits_dev": (3,),
            "urhgpu_msg_records_dev": (2, 5, 7), "urhgpu_blob_capacity": (0, 1, 2, 3, 4), "urhgpu_outputs_to_host": (2,),
            "urhgpu_stream_create": (1, 3, 4, 5), "urhgpu_stream_set_msg_records": (1, 2), "urhgpu_stream_set_auto_noise": (1,),
            "urhgpu_stream_set_auto_center": (1, 2), "urhgpu_stream_push": (2,)}


def to_dev(pipe, iq):
    import torch
    return torch.from_numpy(np.array(iq)).to(pipe.device)


def alternating(n=8193):
    """a carrier whose frequency changes its sign with every sample: with tolerance 0 a pulse-table row per sample"""
    ph = np.cumsum(np.where(np.arange(n) % 2 == 0, 0.5, -0.5))
    return np.stack([np.cos(ph), np.sin(ph)], axis=1).astype(np.float32)


def bases():
    """name -> (capture, params, options of the pass, tuning of the context)"""
    fsk, noisy = cc.params("FSK", np.float32), nc.params("FSK", 1, noise=0.7)
    quiet = nc.capture(1001, 8193)
    tie = synth_fsk(8193, sps=cc.SPS, seed=6, noise=0.05, pause_every=2500, pause_len=700, deviation_hz=20e3)
    return {
        "plain": (cc.capture(3000, np.float32), fsk, {}, None),
        "no_qad": (cc.capture(3000, np.float32), fsk, dict(want_qad=False), None),
        "center_flag_1": (cc.capture(3000, np.float32), fsk, dict(auto_center=True), None),
        "center_flag_0": (np.full((5000, 2), 0.5, np.float32), cc.params("ASK", np.float32, noise=0.1), dict(auto_center=True), None),
        "center_flag_2": (cc.capture(8191, np.int16), cc.params("FSK", np.int16), dict(auto_center=True, center_max_size=7500), {"auto_center_max_bins": 8}),
        "center_flag_3": (tie, cc.params("FSK", np.float32, noise=0.3), dict(auto_center=True, center_max_size=7500), None),
        "noise_flag_1": (quiet, noisy, dict(auto_noise=True), None),
        "noise_flag_2": (nc.capture(4000, 8193, sigma=1.5, amp=3.0), noisy, dict(auto_noise=True), None),
        "noise_and_center": (quiet, noisy, dict(auto_noise=True, auto_center=True), None),
        "dc_correction": (dc_cases.generic(np.float32, 3000), fsk, dict(dc_correction=True), None),
    }


VARIANTS = {"alone": None, "records_pos": True, "records_no_pos": False}        # message records: are the positions shipped


def with_variant(p, options, ship_pos):
    if ship_pos is None:
        return p, options
    return dataclasses.replace(p, write_bit_sample_pos=ship_pos), dict(options, msg_records=True, message_length_divisor=DIVISOR)


def one_shot(rec, iq, p, options, tuning):
    from urh_amd.pipeline import DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0, tuning=tuning)
    res = pipe.iq_to_bits(to_dev(pipe, iq), p, **options)
    results = [list(res.host_counts()), res.noise_flag, res.center_flag]
    res.check_capacity()
    res.host().check()
    if options.get("msg_records"):
        results.append(len(res.message_data()))
    return trace(rec, pipe, results)


def streamed(rec, iq, p, options, tuning):
    from urh_amd.pipeline import DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0, tuning=tuning)
    options = dict(options)
    want_qad = options.pop("want_qad", True)
    st = pipe.stream(len(iq), p, want_qad=want_qad, want_pos=p.write_bit_sample_pos, dtype=iq.dtype, **options)
    devs = [to_dev(pipe, iq) for _ in range(4)]
    results = []

    def keep(r):
        if r is not None:
            r.check()
            results.append([r.seq, r.n_rows, r.n_msg, r.n_bits, r.n_pos, getattr(r, "noise_flag", None), getattr(r, "center_flag", None)])
            if options.get("msg_records"):
                results[-1].append(len(r.message_data()))
    for d in devs:
        keep(st.push(d))
    for r in st.flush():
        keep(r)
    st.close()
    return trace(rec, pipe, results)


def read(res):
    out = [list(res.host_counts()), res.noise_flag, res.center_flag]
    res.check_capacity()
    res.host().check()
    return out


def pipelined(rec, slots):
    from urh_amd.pipeline import DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0, pipelined=True)
    dev, p = to_dev(pipe, cc.capture(4097, np.float32)), cc.params("ASK", np.float32)
    passes = [pipe.iq_to_bits(dev, p, want_qad=True, slot=slot, auto_center=True) for slot in slots]
    return trace(rec, pipe, [read(res) for res in passes])


def sliced(rec, compute_pos):
    from urh_amd.pipeline import DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0)
    p = cc.params("FSK", np.float32, write_pos=False)
    qad = pipe.afp_demod(to_dev(pipe, cc.capture(3000, np.float32)), p)
    return trace(rec, pipe, read(pipe.qad_to_bits(qad, p, compute_pos=compute_pos)))


def checked(rec):
    from urh_amd.pipeline import DemodParams, DevicePipeline
    rec.log = []
    pipe = DevicePipeline(0)
    res = pipe.iq_to_bits_checked(to_dev(pipe, alternating()), DemodParams("FSK", 1, 0.0, 0.0, 1.0, 0, 100, 0.1, 8, True))
    return trace(rec, pipe, read(res))


def protocol_twice(rec):
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.signal import Signal
    rec.log = []
    pipe = DevicePipeline(0)
    g = mc.load()["pad"]
    s = Signal(None, pipe=pipe)
    s.iq = g["iq"]
    for k in ("modulation_type", "bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
              "costas_loop_bandwidth"):
        setattr(s, k, g["meta"][k])
    s.message_length_divisor = DIVISOR
    return trace(rec, pipe, [len(s.get_protocol()), len(s.get_protocol())])


def single_rank(rec):
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    rec.log = []
    eng = GpuShardEngine(0, pipelined=True, host_results=True)
    sp = ShardedPipeline(eng, ThreadComm(ThreadComm.Shared(1), 0))
    res = sp.iq_to_bits(to_dev(eng, cc.capture(8193, np.float32)), cc.params("FSK", np.float32), want_qad=True)
    res.host().check()
    return trace(rec, eng, [list(res.host_counts())])


def scenarios():
    """name -> a function of the recorder that runs the scenario and returns its trace"""
    out = {}
    for base, (iq, p, options, tuning) in bases().items():
        for variant, ship_pos in VARIANTS.items():
            pv, ov = with_variant(p, options, ship_pos)
            out[f"one_shot/{base}/{variant}"] = lambda rec, a=(iq, pv, ov, tuning): one_shot(rec, *a)
            out[f"stream/{base}/{variant}"] = lambda rec, a=(iq, pv, ov, tuning): streamed(rec, *a)
    out["pipelined/same_slot"] = lambda rec: pipelined(rec, (1, 1))
    out["pipelined/two_slots"] = lambda rec: pipelined(rec, (1, 2))
    out["qad_to_bits/alone"] = lambda rec: sliced(rec, False)
    out["qad_to_bits/compute_pos"] = lambda rec: sliced(rec, True)
    out["iq_to_bits_checked/second_pass"] = checked
    out["signal/get_protocol_twice"] = protocol_twice
    out["shard_engine/single_rank"] = single_rank
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


@pytest.mark.parametrize("part", ["calls", "bufs", "pinned", "results"])
def test_passes_equal_the_recorded_traces(traces, recorded, part):
    for name in sorted(recorded):
        assert traces[name][part] == recorded[name][part], (name, part)


def names(t):
    return [c.split()[0] for c in t["calls"]]


def test_the_recorded_traces_hold_the_cases(recorded):
    """no GPU needed beyond the module's mark: the grounds the scenarios were chosen for are in the fixture itself"""
    for route in ("one_shot", "stream"):
        for variant in VARIANTS:
            def flags(base):
                r = recorded[f"{route}/{base}/{variant}"]["results"]
                return (r[1], r[2]) if route == "one_shot" else (r[0][5], r[0][6])
            assert flags("plain") == (None, None) and flags("no_qad") == (None, None)
            for k in (1, 0, 2, 3):
                assert flags(f"center_flag_{k}") == (None, k), (route, variant, k)
            assert flags("noise_flag_1") == (1, None) and flags("noise_and_center") == (1, 1)
            assert flags("noise_flag_2")[0] == 2
            assert len(recorded[f"stream/plain/{variant}"]["results"]) == 4
    # every flavour of a pass through its own entry point, once
    entry = {"plain": "urhgpu_iq_to_bits_dev", "center_flag_1": "urhgpu_iq_to_bits_auto_center_dev", "noise_flag_1": "urhgpu_iq_to_bits_auto_dev",
             "noise_and_center": "urhgpu_iq_to_bits_auto_dev"}
    for base, fn in entry.items():
        called = [c for c in names(recorded[f"one_shot/{base}/alone"]) if c.startswith("urhgpu_iq_to_bits")]
        assert called == [fn], (base, called)
    # the host's decisions slice again; what the device decided does not
    for base, again in (("center_flag_1", 0), ("center_flag_0", 0), ("center_flag_2", 1), ("center_flag_3", 1), ("noise_flag_1", 0), ("noise_flag_2", 1)):
        assert names(recorded[f"one_shot/{base}/alone"]).count("urhgpu_ppseq_to_bits_dev") == again, base
        assert names(recorded[f"stream/{base}/alone"]).count("urhgpu_ppseq_to_bits_dev") == 4 * again, base
        assert names(recorded[f"one_shot/{base}/records_no_pos"]).count("urhgpu_msg_records_dev") == 1 + again, base
    assert "urhgpu_grab_pulse_lens_dev 2 2" in recorded["one_shot/noise_flag_2/alone"]["calls"]               # (the slicing of zeros(2))
    assert names(recorded["iq_to_bits_checked/second_pass"]).count("urhgpu_iq_to_bits_dev") == 2
    assert names(recorded["signal/get_protocol_twice"]).count("urhgpu_msg_records_dev") == 1
    assert names(recorded["pipelined/same_slot"]).count("urhgpu_ctx_join") > names(recorded["pipelined/two_slots"]).count("urhgpu_ctx_join")
    assert "('dc', 0)" in recorded["one_shot/dc_correction/alone"]["bufs"] and "('records', 0)" in recorded["one_shot/plain/records_pos"]["pinned"]
    assert "pos" in recorded["one_shot/plain/records_no_pos"]["bufs"] and "q0:pos" in recorded["qad_to_bits/compute_pos"]["bufs"]
    assert "q0:pos" not in recorded["qad_to_bits/alone"]["bufs"]
    assert any(c.startswith("urhgpu_shard_") for c in names(recorded["shard_engine/single_rank"]))


if __name__ == "__main__":
    first, second = all_traces(), all_traces()
    unstable = sorted(name for name in first if first[name] != second[name])
    assert not unstable, unstable                                # a scenario that is not the same twice is no fixture
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(first, indent=0, sort_keys=True) + "\n")
