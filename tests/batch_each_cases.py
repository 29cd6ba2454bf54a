"""Shared by tests/golden/make_batch_each_golden.py and tests/test_batch_each_golden_gpu.py: where the recording of the real reference on the
sessions of tests/batch_estimate_cases.py lies and how its entries read."""
import json
import os
import struct

from conftest import ROOT

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "batch_each")
GOLDEN = os.path.join(GOLDEN_DIR, "batch_each.json")
SAMPLE_RATE = 2e6
TIMESTAMP_STEP = 10.25                 # capture k of a session was recorded at k * TIMESTAMP_STEP


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)


def demod_params(d):
    """a recorded parameter dict as DemodParams"""
    from urh_amd.pipeline import DemodParams
    return DemodParams(d["modulation_type"], d["bits_per_symbol"], d["noise_threshold"], d["center"], d["center_spacing"], d["tolerance"],
                       d["samples_per_symbol"], d["costas_loop_bandwidth"], d["pause_threshold"], True)


def bits64(x):
    return struct.pack(">d", float(x)).hex()


def assert_messages(got, want, what):
    """a list of protocol.MessageData against the recorded messages: bit string, pause, RSSI and timestamp by their bit patterns, first position"""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, w) in enumerate(zip(got, want)):
        assert "".join(map(str, a.plain_bits)) == w["bits"] and int(a.pause) == w["pause"], (what, i)
        assert bits64(a.rssi) == w["rssi"], (what, i, a.rssi)
        assert int(a.bit_sample_pos[0]) == w["first"] and bits64(a.timestamp) == w["timestamp"], (what, i)
