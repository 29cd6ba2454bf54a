#!/usr/bin/env python3
"""Run the REAL reference (this container only) on the seeded captures of tests/noise_cases.py with its default setting
default_noise_threshold = "automatic": AutoInterpretation.detect_noise_level on IQArray.magnitudes (Signal.py:97-103), then
ProtocolAnalyzer.get_protocol_from_signal with that threshold.  Per case the fixture keeps the recipe (seed and parameters -- never the
capture), the threshold as a hex float64, the messages' bits and their pauses.  -> tests/golden/auto_noise.json

PSK captures: the reference's Costas loop never writes result[0] (np.empty: uninitialised memory); as in make_messages_golden.py,
numpy.empty hands out float32 arrays filled with -4.0 for them, the value the library documents for that element.

    python tests/golden/make_auto_noise_golden.py
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

import noise_cases as nc  # noqa: E402

out = {}
_empty = np.empty
for name, kw in nc.pass_cases().items():
    iq = np.array(nc.case_capture(kw))
    p = nc.params(kw["mod"], kw["bits_per_symbol"])
    if kw["mod"] == "PSK":
        def _filled(shape, dtype=float, *a, **k):
            arr = _empty(shape, dtype, *a, **k)
            if np.dtype(dtype) == np.float32:
                arr.fill(-4.0)
            return arr
        np.empty = _filled
    s = Signal("")
    s.iq_array = IQArray(iq)
    s.noise_threshold = AutoInterpretation.detect_noise_level(s.iq_array.magnitudes)        # what Signal.__init__ does for "automatic"
    s.modulation_type = p.modulation_type
    s.bits_per_symbol = p.bits_per_symbol
    s.center = p.center
    s.center_spacing = p.center_spacing
    s.tolerance = p.tolerance
    s.samples_per_symbol = p.samples_per_symbol
    s.pause_threshold = p.pause_threshold
    s.costas_loop_bandwidth = p.costas_loop_bandwidth
    pa = ProtocolAnalyzer(s)
    pa.get_protocol_from_signal()
    np.empty = _empty
    thr = float(s.noise_threshold)
    out[name] = dict(recipe=kw, threshold=thr.hex(), gates_all=not (thr < s.max_magnitude), bits=[m.plain_bits_str for m in pa.messages],
                     pauses=[int(m.pause) for m in pa.messages])
    print(name, thr, len(pa.messages), sum(len(b) for b in out[name]["bits"]))
with open(nc.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=0, sort_keys=True)
print(os.path.getsize(nc.GOLDEN), "bytes")
