#!/usr/bin/env python3
"""Run the REAL reference's afp_demod and grab_pulse_lens (oracle/_ref, where the reference is) on a named subset of the batch's edge
inputs (tests/batch_edge_cases.py; the subset: tests/test_batch_edges_host.py::golden_cases) and store the outputs in
tests/golden/batch_edge/batch_edge.npz: what pins the oracle on denormal amplitudes, non-finite samples at the batch's step seams, gate
ties, the ends of the integer ranges and threshold-equal values where the reference is absent.

The float32 captures built on edge_inputs.base_capture are seeded and quantised: they are stored as the CRC-32 of their bytes, and the
host test rebuilds them and checks the CRC before it compares.  The small integer and lattice captures, whose builders take nearest
angles, are stored themselves.  Arrays only.

    python tests/golden/make_batch_edge_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import build_ref  # noqa: E402
import edge_inputs as E  # noqa: E402
from test_batch_edges_host import golden_cases  # noqa: E402


def main():
    from urh_amd.batch import batch_step
    sf, _, _ = build_ref.import_ref()
    S = batch_step()
    out, names = {"step": np.int64(S)}, []
    with np.errstate(all="ignore"):
        for name, b, iq, with_input in golden_cases(S):
            qad = np.asarray(sf.afp_demod(iq, b.noise, b.mod, 2 ** b.bps)).copy()
            out[name + "/qad"] = qad
            out[name + "/pp"] = np.asarray(sf.grab_pulse_lens(qad, b.center, b.tol, b.mod, b.sps, b.bps, b.spacing)).copy()
            out[name + "/crc"] = np.uint32(E.crc(iq))
            out[name + "/noise"], out[name + "/center"] = np.float64(b.noise), np.float64(b.center)
            if with_input:
                out[name + "/iq"] = iq
            names.append(name)
    out["names"] = np.array(names)
    path = os.path.join(HERE, "batch_edge", "batch_edge.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
