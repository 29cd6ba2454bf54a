#!/usr/bin/env python3
"""Run the REAL reference (where it is built) on the captures of tests/batch_auto_cases.py: AutoInterpretation.detect_noise_level on
IQArray.magnitudes, what Signal(filename) does for every file it opens with default_noise_threshold = "automatic" (Signal.py:97-103).
The fixture keeps data only -- per sample type the thresholds of the size sweep as hex float64, and those of the flag captures (the
exception's name where the reference raises); never a capture.  -> tests/golden/batch_auto/batch_auto.json

    python tests/golden/make_batch_auto_golden.py
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

import batch_auto_cases as bc  # noqa: E402
import noise_cases as nc  # noqa: E402


def threshold(iq):
    try:
        return float(AutoInterpretation.detect_noise_level(IQArray(np.array(iq)).magnitudes)).hex()
    except (ValueError, OverflowError) as exc:
        return type(exc).__name__


out = {"lengths": list(bc.SWEEP_LENGTHS), "sweep": {}, "flags": {}}
for dt in nc.DTYPES5:
    name = np.dtype(dt).name
    out["sweep"][name] = [threshold(iq) for iq in bc.sweep(dt)]
    print(name, sum(1 for t in out["sweep"][name] if float.fromhex(t) != 0.0), "non-zero")
out["flags"]["float32"] = {name: threshold(iq) for name, iq in bc.flag_captures_f32()}
out["flags"]["int8"] = {name: threshold(iq) for name, iq in bc.flag_captures_i8()}
print(out["flags"])
os.makedirs(os.path.dirname(bc.GOLDEN), exist_ok=True)
with open(bc.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=0, sort_keys=True)
print(os.path.getsize(bc.GOLDEN), "bytes")
