#!/usr/bin/env python3
"""Run the REAL reference (where it is built) on the gain sweep of tests/batch_center_cases.py, each capture the way the reference opens
a file and interprets it: noise_threshold = AutoInterpretation.detect_noise_level(magnitudes) (Signal.py:97-103), center =
AutoInterpretation.detect_center(signal.qad, max_size) (the configured center where it gives None), ProtocolAnalyzer's messages.
The fixture keeps data only -- per (modulation, sample type, max_size) and capture the center as float.hex (null: None), the class
center_cases.expected gives for the reference's demodulated signal, and a hash of the messages' bits and pauses; never a capture.
The same for batch_auto_cases.flag_captures_f32 ("flags": by name; the exception's name where detect_noise_level raises) -- among them
the constant envelope, whose histogram has 166 million bins: the reference takes minutes over it, which is why it is recorded here.
-> tests/golden/batch_center/batch_center.json

    python tests/golden/make_batch_center_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_python  # noqa: E402

ref_python.setup()
from urh.ainterpretation import AutoInterpretation  # noqa: E402
from urh.signalprocessing.IQArray import IQArray  # noqa: E402
from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer  # noqa: E402
from urh.signalprocessing.Signal import Signal  # noqa: E402

import batch_auto_cases as bac  # noqa: E402
import batch_center_cases as B  # noqa: E402
import noise_cases as nc  # noqa: E402
import center_cases as cc  # noqa: E402


def interpret(iq, p, max_size):
    s = Signal("")
    s.iq_array = IQArray(np.array(iq))
    try:
        s.noise_threshold = AutoInterpretation.detect_noise_level(s.iq_array.magnitudes)
    except (ValueError, OverflowError) as exc:
        return (type(exc).__name__, None, None, None)
    s.modulation_type = p.modulation_type
    s.bits_per_symbol = p.bits_per_symbol
    s.center_spacing = p.center_spacing
    s.tolerance = p.tolerance
    s.samples_per_symbol = p.samples_per_symbol
    s.pause_threshold = p.pause_threshold
    qad = np.array(s.qad)
    c = AutoInterpretation.detect_center(qad, max_size=max_size)
    s.center = p.center if c is None else c
    pa = ProtocolAnalyzer(s)
    pa.get_protocol_from_signal()
    return (float(s.noise_threshold).hex(), None if c is None else float(c).hex(), cc.expected(qad, max_size),
            B.bits_hash([m.plain_bits_str for m in pa.messages], [int(m.pause) for m in pa.messages]))


out = {}
for mod in B.GAIN_MODS:
    p = B.gain_params(mod)
    for dt in B.GAIN_DTYPES:
        for max_size in B.GAIN_MAX_SIZES:
            key = "%s/%s/%s" % (mod, np.dtype(dt).name, max_size)
            rows = [interpret(iq, p, max_size) for iq in B.gain_sweep(mod, dt)]
            out[key] = {"center": [r[1] for r in rows], "class": [r[2] for r in rows], "hash": [r[3] for r in rows]}
            print(key, {c: out[key]["class"].count(c) for c in ("ok", "none", "tie", "wide")})
out["flags"] = {}
for name, iq in bac.flag_captures_f32():
    r = interpret(iq, nc.params("FSK", 1, write_pos=False), None)
    out["flags"][name] = {"noise": r[0], "center": r[1], "class": r[2], "hash": r[3]}
    print(name, out["flags"][name])
os.makedirs(os.path.dirname(B.GOLDEN), exist_ok=True)
with open(B.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=0, sort_keys=True)
print(os.path.getsize(B.GOLDEN), "bytes")
