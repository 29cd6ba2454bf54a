"""The fixtures of tests/golden/msg_records/msg_records.npz / .json (tests/golden/make_msg_records_golden.py wrote them with the real reference's
ProtocolAnalyzer.get_protocol_from_signal): loading, and the comparison of a list of protocol.MessageData with one of them."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def load():
    """{case: dict(iq=..., meta=..., want={divisor: dict(bits, msg_off, pauses, pos, pos_off, rssi, timestamp)})}"""
    if not _cache:
        z = np.load(os.path.join(GOLDEN, "msg_records", "msg_records.npz"))
        meta = json.load(open(os.path.join(GOLDEN, "msg_records", "msg_records.json")))
        for name, m in meta.items():
            want = {int(d): {k: z[f"{name}|{d}/{k}"] for k in ("bits", "msg_off", "pauses", "pos", "pos_off", "rssi", "timestamp")} for d in m["divisors"]}
            _cache[name] = dict(iq=z[f"{name}/iq"], meta=m, want=want)
    return _cache


def names():
    return sorted(load())


def pairs():
    """every (case, divisor)"""
    return [(n, int(d)) for n in names() for d in load()[n]["meta"]["divisors"]]


def params(meta, want_pos=True):
    from urh_amd.pipeline import DemodParams
    return DemodParams(meta["modulation_type"], meta["bits_per_symbol"], meta["noise_threshold"], meta["center"], meta["center_spacing"],
                       meta["tolerance"], meta["samples_per_symbol"], meta["costas_loop_bandwidth"], meta["pause_threshold"], want_pos)


def same_float(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def assert_messages(got, want, what):
    """got: list of protocol.MessageData; want: one fixture entry.  Bits, pauses, positions, RSSI (== or both NaN) and timestamp."""
    off, poff = want["msg_off"], want["pos_off"]
    assert len(got) == len(want["pauses"]), (what, len(got), len(want["pauses"]))
    for m, g in enumerate(got):
        assert list(g.plain_bits) == want["bits"][off[m]:off[m + 1]].tolist(), (what, m)
        assert g.pause == int(want["pauses"][m]), (what, m, g.pause)
        assert list(g.bit_sample_pos) == want["pos"][poff[m]:poff[m + 1]].tolist(), (what, m)
        assert same_float(float(g.rssi), float(want["rssi"][m])), (what, m, g.rssi, float(want["rssi"][m]))
        assert g.timestamp == float(want["timestamp"][m]), (what, m)
