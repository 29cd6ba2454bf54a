#!/usr/bin/env python3
"""Run the REAL reference's afp_demod / grab_pulse_lens / _ppseq_to_bits (oracle/_ref, this container only) on the edge-value inputs of
tests/edge_inputs.py and store the outputs in tests/golden/edge/edge.npz: what pins the oracle on NaN / inf / extreme samples, on
amplitudes scaled by 2^k and on samples exactly on the noise gate where the reference is absent.

One capture per modulation and value class at the default lengths: sprinkled (variant 0) and scaled (k = -20) as float32, the tie
captures as int8 and float32, PSK also with the NaN inside a gated stretch.  A float32 capture and its output together would not fit
the size limit of a committed file (they are noise: nothing compresses), so the large captures are stored as the CRC-32 of their
bytes -- the builders are seeded and quantised, tests/test_edge_values_host.py rebuilds them and checks the CRC before it compares --
and only the small tie captures and the pulse-table inputs are stored themselves.  Arrays only.

    python tests/golden/make_edge_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import build_ref  # noqa: E402
import edge_inputs as E  # noqa: E402
import ref_python  # noqa: E402


def main():
    sf, _, _ = build_ref.import_ref()
    ref_python.setup()
    from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer
    pa = ProtocolAnalyzer(None)
    out, names = {}, []
    with np.errstate(all="ignore"):
        for name, mod, order, iq, noise, with_input in E.golden_demod_cases():
            qad = np.asarray(sf.afp_demod(iq, noise, mod, order)).copy()
            if mod == "PSK":
                qad[0] = -4.0                                  # the reference leaves it unwritten (np.empty)
            out[name + "/qad"] = qad
            out[name + "/crc"] = np.uint32(E.crc(iq))
            out[name + "/noise"] = np.float64(noise)
            if with_input:
                out[name + "/iq"] = iq
            names.append(name)
        for name, mod, bps, x, center, spacing, tol in E.golden_rect_cases():
            pp = np.asarray(sf.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing)).copy()
            out[name + "/x"], out[name + "/pp"] = x, pp
            flat = E.flatten_messages(*pa._ppseq_to_bits(pp, 40, bps, pause_threshold=8))
            for key, a in zip(("bits", "msg_off", "pauses", "pos", "pos_off"), flat):
                out[name + "/" + key] = a
            names.append(name)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "edge", "edge.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
