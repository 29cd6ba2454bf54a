#!/usr/bin/env python3
"""Run the REAL reference's DC correction (oracle/_ref + the reference's Python classes, this container only) on captures of the
reference's tests/data and store inputs + outputs in tests/golden/dc/<name>.npz:

    iq          the capture (cropped), in its sample type
    work        Filter([], FilterType.dc_correction).work(iq) stored into an IQArray of the capture's type (the cast every caller applies)
    start, end, noise_threshold, modulation_type
    range_iq    the samples after Signal.filter_range(start, end, that filter)
    range_qad   Signal._qad after it

    python tests/golden/make_dc_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_python  # noqa: E402

# name, file under the reference's tests/data, sample type, samples kept, modulation, noise threshold, range
CASES = [
    ("ask_f32", "ask.complex", np.float32, 13_000, "ASK", 0.02, (1_003, 9_778)),
    ("fsk_f32", "fsk.complex", np.float32, 24_000, "FSK", 0.01, (0, 24_000)),
    ("homematic_i16", "homematic.complex32s", np.int16, 24_000, "FSK", 300.0, (4_099, 20_001)),
    ("two_participants_i8", "two_participants.complex16s", np.int8, 30_000, "FSK", 3.0, (7, 28_672)),
]


def main():
    ref_python.setup()
    from urh.signalprocessing.Filter import Filter, FilterType
    from urh.signalprocessing.IQArray import IQArray
    from urh.signalprocessing.Signal import Signal
    data = os.path.join(ref_python.REF_ROOT, "tests", "data")
    os.makedirs(os.path.join(HERE, "dc"), exist_ok=True)
    for name, fname, dtype, keep, mod, noise, (start, end) in CASES:
        iq = np.fromfile(os.path.join(data, fname), dtype=dtype).reshape(-1, 2)[:keep].copy()
        assert len(iq) == keep, (name, len(iq))
        flt = Filter([], FilterType.dc_correction)
        whole = IQArray(iq.copy())
        whole[0:keep] = flt.work(whole[0:keep])
        sig = Signal("")
        sig.iq_array = IQArray(iq.copy())
        sig.modulation_type = mod
        sig.noise_threshold = noise
        _ = sig.qad
        sig.filter_range(start, end, flt)
        np.savez_compressed(os.path.join(HERE, "dc", name + ".npz"), iq=iq, work=whole.data, start=start, end=end, noise_threshold=noise,
                            modulation_type=mod, range_iq=sig.iq_array.data, range_qad=np.asarray(sig._qad))
        print(name, iq.dtype, len(iq), "mean", np.mean(iq, axis=0))


if __name__ == "__main__":
    main()
