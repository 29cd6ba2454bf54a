#!/usr/bin/env python3
"""Run the REAL reference's signal_functions.fir_filter / iir_filter (oracle/_ref, where the reference is built) on the inputs of
tests/filter_cases.py and store inputs + outputs in tests/golden/filter/edges.npz: the IIR family (sizes at max(M, N + 1), non-finite
samples and coefficients), empty taps, the 2^60 threshold pair and 4001 taps on 1000 samples.

    python tests/golden/make_filter_edges_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import build_ref  # noqa: E402
import filter_cases as F  # noqa: E402


def main():
    sf, _, _ = build_ref.import_ref()
    out = {}
    with np.errstate(all="ignore"):
        fir = [(name, x, h, np.asarray(sf.fir_filter(x, h))) for name, x, h in F.golden_fir_cases()]
        iir = [(name, a, b, x, np.asarray(sf.iir_filter(a, b, x))) for name, a, b, x in F.d_cases()]
        empty = []
        for name, x, h in F.e_cases():
            kind, y = F.fir_outcome(sf.fir_filter, x, h)
            empty.append((name, x, h, kind, y if y is not None else np.zeros(0, np.complex64)))
    for sec, rows, cols in (("fir", fir, (("x", 1, np.complex64), ("h", 2, np.complex64), ("y", 3, np.complex64))),
                            ("iir", iir, (("a", 1, np.float64), ("b", 2, np.float64), ("x", 3, np.complex64), ("y", 4, np.complex64))),
                            ("empty", empty, (("x", 1, np.complex64), ("h", 2, np.complex64), ("y", 4, np.complex64)))):
        out[sec + "_names"] = np.array([r[0] for r in rows])
        for key, col, dtype in cols:
            out[f"{sec}_{key}"], out[f"{sec}_{key}_off"] = F.pack([r[col] for r in rows], dtype)
    out["empty_kind"] = np.array([r[3] for r in empty])
    np.savez_compressed(F.GOLDEN, **out)
    print("wrote", len(fir), "FIR,", len(iir), "IIR,", len(empty), "empty-taps cases:", os.path.getsize(F.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
