#!/usr/bin/env python3
"""tools/batch_auto_probe.py [--out profiles/batch_auto_probe.txt] [--sets a,lo,hi] [--rounds 5]

A batch of captures that detects every capture's noise threshold (DevicePipeline.iq_to_bits_batch_auto: four launches, three read-backs)
against the fastest route to the same results before it, and against the batch with one fixed threshold:

    A  iq_to_bits_batch_auto
    B  a pipelined CaptureStream(auto_noise=True), push_upload per capture + flush
    C  iq_to_bits_batch with p.noise_threshold fixed: what the detection adds is A - C

One MI355X, one process, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: float32 2-FSK bursts
with quiet chunks (tests/noise_cases.capture), gains cycled over STREAM_GAINS, pinned host arrays; the thresholds, bits and pulse tables
of A and B are compared before anything is timed.

    set (a)   4096 captures of 16 384 samples (DESIGN.md 7.7e's set)
    set (lo)  512 of 131 072      set (hi)  256 of 262 144: either side of batch.LONG_FROM_DEFAULT, to see where A and B cross

--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/batch_auto_probe.py --only-batch --sets a)."""
import argparse
import os
import statistics
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = {"a": (4096, 16384), "lo": (512, 131072), "hi": (256, 262144)}
DISTINCT = 8                 # different captures per set, one per gain
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass
FIXED = 0.02                 # path C's threshold


def captures(k, n):
    import torch
    import noise_cases as nc
    base = []
    for s in range(min(DISTINCT, k)):
        sigma, amp = nc.STREAM_GAINS[s % len(nc.STREAM_GAINS)]
        base.append(torch.from_numpy(np.array(nc.capture(8000 + s, n, sigma=sigma, amp=amp))).pin_memory())
    return [base[i % len(base)] for i in range(k)]


class Paths:
    def __init__(self, pipe, p, caps, n):
        import torch
        self.pipe, self.p, self.caps, self.n = pipe, p, caps, n
        self.np_caps = [c.numpy() for c in caps]
        self.stream = pipe.stream(n, p, want_qad=False, want_pos=False, auto_noise=True)
        self.slots = [torch.empty((n, 2), dtype=torch.float32, device=pipe.device) for _ in range(4)]

    def a(self):
        return self.pipe.iq_to_bits_batch_auto(self.np_caps, self.p, long_from=NEVER)

    def c(self):
        return self.pipe.iq_to_bits_batch(self.np_caps, replace(self.p, noise_threshold=FIXED), long_from=NEVER)

    def b(self, keep=None):
        n_out = 0

        def take(r):
            if keep is not None:
                keep[r.seq] = (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated), float(r.noise_threshold), int(r.noise_flag))
        for i, c in enumerate(self.caps):
            r = self.stream.push_upload(c, self.slots[i % 4])
            if r is not None:
                n_out += 1
                take(r)
        for r in self.stream.flush():
            n_out += 1
            take(r)
        assert n_out == len(self.caps)

    def verify(self):
        keep = {}
        self.b(keep)
        seq0 = min(keep)
        res = self.a()
        assert len(res) == len(self.caps)
        n_trunc = 0
        for i, h in enumerate(res):
            pp, bits, off, pauses, trunc, thr, flag = keep[seq0 + i]
            assert res.noise[i] == thr and res.noise_flags[i] == flag == 1, (i, res.noise[i], thr, flag)
            if trunc or h.truncated:                         # (the two routes size their rows differently; a truncated result is not compared)
                n_trunc += 1
                continue
            assert np.array_equal(h.bits(), bits) and np.array_equal(h.ppseq(), pp) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
        return sum(h.n_bits for h in res), n_trunc, sorted(set(res.noise))

    def close(self):
        self.stream.close()


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} - {max(v):.2f})"


def measure(pipe, p, k, n, rounds, out):
    from urh_amd.batch import launch_counts
    dev = pipe.device
    paths = Paths(pipe, p, captures(k, n), n)
    n_bits, n_trunc, thresholds = paths.verify()
    for fn in (paths.a, paths.b, paths.c):                   # warm-up (buffers grown, pinned memory there)
        timed(fn, dev)
    a, b, c = [], [], []
    for _ in range(rounds):
        before = launch_counts(pipe)
        a.append(timed(paths.a, dev))
        after = launch_counts(pipe)
        b.append(timed(paths.b, dev))
        c.append(timed(paths.c, dev))
    paths.close()
    ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
    line = (f"{k:6d} x {n:8d}  A batch_auto {fmt(a)} ms  B stream auto_noise {fmt(b)} ms  C batch fixed {fmt(c)} ms  B/A {mb / ma:6.2f}  A-C {ma - mc:8.2f} ms"
            f"  A: {k / ma * 1e3:10.0f} captures/s {k * n / ma * 1e3 / 1e9:7.3f} Gsamples/s  launches {after[0] - before[0]} copies {after[1] - before[1]}"
            f"  slowest A < fastest B: {max(a) < min(b)}  bits {n_bits}  truncated (not compared) {n_trunc}  thresholds {thresholds}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_auto_probe.txt"))
    ap.add_argument("--sets", default="a,lo,hi")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    args = ap.parse_args()
    import torch
    import noise_cases as nc
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0, pipelined=True)
    p = nc.params("FSK", 1, write_pos=False)
    if args.only_batch:
        for s in args.sets.split(","):
            k, n = SETS[s]
            caps = [c.numpy() for c in captures(k, n)]
            pipe.iq_to_bits_batch_auto(caps, p, long_from=NEVER)
            ms = timed(lambda: pipe.iq_to_bits_batch_auto(caps, p, long_from=NEVER), pipe.device)
            print(f"set ({s}) {k} x {n}: one batch with automatic noise thresholds {ms:.2f} ms")
        return
    out = [f"# tools/batch_auto_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); launches / copies: of one A",
           "# A = iq_to_bits_batch_auto; B = pipelined CaptureStream(auto_noise=True), push_upload per capture + flush; C = iq_to_bits_batch, threshold "
           f"{FIXED} (host arrays in, results on the host)"]
    for s in args.sets.split(","):
        k, n = SETS[s]
        measure(pipe, p, k, n, args.rounds, out)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
