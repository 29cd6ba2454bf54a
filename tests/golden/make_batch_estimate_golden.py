#!/usr/bin/env python3
"""Run the REAL reference (where it is built) on the captures of tests/batch_estimate_cases.py:
  - auto_interpretation.segment_messages_from_magnitudes on IQArray.magnitudes with the case's threshold, for every geometry case and every
    capture of the many-captures batch  -> tests/golden/batch_estimate/ranges.npz (names, offsets, pairs: data only, never a capture)
  - AutoInterpretation.estimate(capture, noise, modulation) for every capture of every session, with the session's arguments for that
    capture -> tests/golden/batch_estimate/estimates.json (the dict, null, or the exception's type name where the reference raises)
A batch has no Costas loop, so a session must not hold a capture the reference detects as PSK: asserted here (replace such a capture), and
the comparison in tests/test_batch_estimate_gpu.py then leaves no capture out.

    python tests/golden/make_batch_estimate_golden.py
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
from urh.ainterpretation import AutoInterpretation as AI  # noqa: E402
from urh.cythonext import auto_interpretation as c_auto_interpretation  # noqa: E402
from urh.signalprocessing.IQArray import IQArray  # noqa: E402

import batch_estimate_cases as bc  # noqa: E402


def ranges(iq, thr):
    if len(iq) == 0:
        return np.zeros((0, 2), np.int64)
    got = c_auto_interpretation.segment_messages_from_magnitudes(IQArray(np.array(iq)).magnitudes, thr)
    return np.asarray(got, dtype=np.int64).reshape(-1, 2)


names, parts = [], []
for dt in bc.GEOMETRY_DTYPES:
    for name, iq, thr in bc.geometry(dt):
        names.append(f"{np.dtype(dt).name}/{name}")
        parts.append(ranges(iq, thr))
caps, thr = bc.many()
for i, iq in enumerate(caps):
    names.append(f"many/{i}")
    parts.append(ranges(iq, thr))
offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
os.makedirs(bc.GOLDEN_DIR, exist_ok=True)
np.savez_compressed(bc.RANGES, names=np.array(names), offsets=offsets, pairs=np.concatenate(parts).astype(np.int64))
print(len(names), "captures,", int(offsets[-1]), "ranges,", os.path.getsize(bc.RANGES), "bytes")

out = {}
for sname, s in bc.sessions().items():
    k = len(s["captures"])
    noise, mods = bc.per_capture(s["noise"], k), bc.per_capture(s["modulation"], k)
    res = []
    for iq, nz, m in zip(s["captures"], noise, mods):
        iq = np.array(iq)
        try:
            if m is None and len(iq):
                arr = IQArray(iq)
                thr_c = AI.detect_noise_level(arr.magnitudes) if nz is None else nz
                seen = AI.detect_modulation_for_messages(arr, AI.segment_messages_from_magnitudes(arr.magnitudes, noise_threshold=thr_c))
                assert seen != "PSK", f"{sname}: the reference detects PSK for a capture: replace it (a batch has no Costas loop)"
            r = AI.estimate(iq, noise=nz, modulation=m)
            res.append(None if r is None else {key: (float(v) if key in ("center", "noise") else (int(v) if key != "modulation_type" else v))
                                               for key, v in r.items()})
        except (ValueError, OverflowError) as exc:
            res.append(type(exc).__name__)
    out[sname] = res
    print(sname, res)
with open(bc.ESTIMATES, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
print(os.path.getsize(bc.ESTIMATES), "bytes")
