#!/usr/bin/env python3
"""Run the REAL reference (where it is importable through oracle/ref_python.py) on every capture of every session of
tests/batch_estimate_cases.py the way it opens a file of a recording session: a Signal of its own with the reference's default parameters,
the session's noise threshold and modulation for that capture where it gives them, Signal.auto_detect (detecting what the session does not
give), then ProtocolAnalyzer.get_protocol_from_signal.
    -> tests/golden/batch_each/batch_each.json   per session and capture: the Signal's parameters BEFORE auto_detect ("base") and after it
       ("params"), what auto_detect returned, the arguments it handed AutoInterpretation.estimate ("noise_arg", "modulation_arg"), and per
       message the bit string, the pause, the RSSI's bit pattern (hex of the float64) and the first position; or the type name of the
       exception the reference raises
Data only, never a capture.  A batch with a parameter set per capture has no Costas loop: asserted here that the reference ends with PSK for
no capture, so the comparison in tests/test_batch_each_golden_gpu.py leaves no capture out.

    python tests/golden/make_batch_each_golden.py
"""
import json
import os
import struct
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_python  # noqa: E402

ref_python.setup()
from urh.signalprocessing.IQArray import IQArray  # noqa: E402
from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer  # noqa: E402
from urh.signalprocessing.Signal import Signal  # noqa: E402

import batch_each_cases as ec  # noqa: E402
import batch_estimate_cases as bc  # noqa: E402

KEYS = ("modulation_type", "bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
        "costas_loop_bandwidth", "message_length_divisor")


def params_of(s):
    out = {}
    for k in KEYS:
        v = getattr(s, k)
        out[k] = v if isinstance(v, str) else (float(v) if k in ("noise_threshold", "center", "center_spacing", "costas_loop_bandwidth") else int(v))
    return out


def interpret(iq, nz, m, timestamp):
    s = Signal("")
    s.iq_array = IQArray(np.array(iq))
    s.sample_rate, s.timestamp = ec.SAMPLE_RATE, timestamp
    if nz is not None:
        s.noise_threshold = nz
    if m is not None:
        s.modulation_type = "ASK" if m == "OOK" else m          # (bits_per_symbol is 1: auto_detect hands "OOK" to the estimate for ASK)
    base = params_of(s)
    entry = dict(base=base, noise_arg=None if nz is None else float(s.noise_threshold),
                 modulation_arg=None if m is None else ("OOK" if s.bits_per_symbol == 1 and s.modulation_type == "ASK" else s.modulation_type))
    entry["detected"] = bool(s.auto_detect(emit_update=False, detect_modulation=m is None, detect_noise=nz is None))
    entry["params"] = params_of(s)
    assert s.modulation_type != "PSK", "the reference ends with PSK for a capture: replace it (this batch has no Costas loop)"
    pa = ProtocolAnalyzer(s)
    pa.get_protocol_from_signal()
    entry["messages"] = [dict(bits="".join(map(str, msg.plain_bits)), pause=int(msg.pause), rssi=struct.pack(">d", float(msg.rssi)).hex(),
                              first=int(msg.bit_sample_pos[0]), timestamp=struct.pack(">d", float(msg.timestamp)).hex()) for msg in pa.messages]
    return entry


def main():
    out = {}
    for sname, s in bc.sessions().items():
        k = len(s["captures"])
        noise, mods = bc.per_capture(s["noise"], k), bc.per_capture(s["modulation"], k)
        res = []
        for i, (iq, nz, m) in enumerate(zip(s["captures"], noise, mods)):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                try:
                    res.append(interpret(iq, nz, m, ec.TIMESTAMP_STEP * i))
                except (ValueError, OverflowError, IndexError, ZeroDivisionError) as exc:
                    res.append(type(exc).__name__)
        out[sname] = res
        print(sname, [r if isinstance(r, str) else (r["params"]["modulation_type"], r["params"]["samples_per_symbol"], len(r["messages"])) for r in res])
    os.makedirs(ec.GOLDEN_DIR, exist_ok=True)
    with open(ec.GOLDEN, "w") as fh:
        json.dump(out, fh, separators=(",", ":"), sort_keys=True)
    print(os.path.getsize(ec.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
