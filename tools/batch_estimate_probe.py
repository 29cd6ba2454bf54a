#!/usr/bin/env python3
"""tools/batch_estimate_probe.py [--out profiles/batch_estimate_probe.txt] [--sets a,lo] [--mods ASK,FSK] [--rounds 5]

The estimate of a session (DevicePipeline.estimate_batch) against the route to the same estimates before it:

    A  estimate_batch over the captures
    B  a loop of estimators.estimate_dev over the same captures

One MI355X, one process, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: float32 ASK and 2-FSK
bursts with quiet chunks (tests/noise_cases.capture), eight different ones per set, resident on the device for both paths (A gathers them
into one buffer itself).  Each set is measured with the modulation given and with the modulation detected; the noise is detected in both.
The estimates of A and B are compared for equality before anything is timed.

    set (a)   4096 captures of 16 384 samples      set (lo)  512 of 131 072

--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/batch_estimate_probe.py --only-batch --sets a --mods FSK)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = {"a": (4096, 16384), "lo": (512, 131072)}
DISTINCT = 8                 # different captures per set
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to estimate_dev


def captures(pipe, k, n, mod):
    import torch
    import noise_cases as nc
    base = [torch.from_numpy(np.array(nc.capture(8300 + s, n, mod))).to(pipe.device) for s in range(min(DISTINCT, k))]
    return [base[i % len(base)] for i in range(k)]


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return set(a) == set(b) and all(a[key] == b[key] if key == "modulation_type" else float(a[key]) == float(b[key]) for key in a)


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} - {max(v):.2f})"


def measure(pipe, mod, given, k, n, rounds, out):
    from urh_amd.batch import launch_counts
    from urh_amd.estimators import estimate_dev
    dev = pipe.device
    caps = captures(pipe, k, n, mod)
    modulation = mod if given else None
    path_a = lambda: pipe.estimate_batch(caps, modulation=modulation, long_from=NEVER)                    # noqa: E731
    path_b = lambda: [estimate_dev(pipe, c, modulation=modulation) for c in caps]                          # noqa: E731
    got, want = list(path_a()), path_b()
    assert len(got) == len(want) == k and all(same(x, y) for x, y in zip(got, want)), "estimate_batch differs from estimate_dev"
    n_est = sum(1 for x in got if x is not None)
    timed(path_a, dev), timed(path_b, dev)                   # warm-up (buffers grown, pinned memory there)
    a, b = [], []
    for _ in range(rounds):
        before = launch_counts(pipe)
        a.append(timed(path_a, dev))
        after = launch_counts(pipe)
        b.append(timed(path_b, dev))
    ma, mb = statistics.median(a), statistics.median(b)
    line = (f"{mod} {'given   ' if given else 'detected'} {k:6d} x {n:8d}  A estimate_batch {fmt(a)} ms  B estimate_dev loop {fmt(b)} ms  B/A {mb / ma:6.2f}  "
            f"A: {ma / k * 1e3:8.1f} us/capture  B: {mb / k * 1e3:8.1f} us/capture  batch launches {after[0] - before[0]} copies {after[1] - before[1]}  "
            f"slowest A < fastest B: {max(a) < min(b)}  estimated {n_est} of {k}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_estimate_probe.txt"))
    ap.add_argument("--mods", default="ASK,FSK")
    ap.add_argument("--sets", default="a,lo")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0)
    mods = args.mods.split(",")
    if args.only_batch:
        for mod in mods:
            for s in args.sets.split(","):
                k, n = SETS[s]
                caps = captures(pipe, k, n, mod)
                pipe.estimate_batch(caps, modulation=mod, long_from=NEVER)
                ms = timed(lambda: pipe.estimate_batch(caps, modulation=mod, long_from=NEVER), pipe.device)
                print(f"{mod} set ({s}) {k} x {n}: one estimate_batch {ms:.2f} ms")
        return
    out = [f"# tools/batch_estimate_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); batch launches / copies: of one A "
           "(urhgpu_batch_launches: noise, segmentation, demodulation; the estimators' native calls are not counted there)",
           "# A = estimate_batch; B = a loop of estimate_dev; captures resident on the device, noise detected, modulation given or detected"]
    for mod in mods:
        for s in args.sets.split(","):
            k, n = SETS[s]
            for given in (True, False):
                measure(pipe, mod, given, k, n, args.rounds, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
