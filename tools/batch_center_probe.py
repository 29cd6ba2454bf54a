#!/usr/bin/env python3
"""tools/batch_center_probe.py [--out profiles/batch_center_probe.txt] [--sets a,lo,hi] [--mods ASK,FSK] [--rounds 5]

A batch of captures that detects every capture's noise threshold AND center (DevicePipeline.iq_to_bits_batch_center) against the fastest
route to the same results before it, and against the batch without a center:

    A  iq_to_bits_batch_center
    B  a pipelined CaptureStream(auto_noise=True, auto_center=True), push_upload per capture + flush
    C  iq_to_bits_batch_auto: no center is detected and every capture is sliced with p.center, so its results are NOT A's -- it is not a
       lower bound of A (A demodulates into a buffer and walks that, C's walk demodulates as it goes), only the cost of the batch before
       the center: what the center adds is about A - C

One MI355X, one process, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: float32 ASK and
2-FSK bursts with quiet chunks (tests/noise_cases.capture), gains cycled over STREAM_GAINS, pinned host arrays; the thresholds, centers,
center flags, bits and pulse tables of A and B are compared before anything is timed.  "host" is the part of one A spent settling the
centers the device left to numpy (estimators.peaks_center is a Python loop per tied capture) and slicing those captures again.

    set (a)   4096 captures of 16 384 samples      set (lo)  512 of 131 072      set (hi)  256 of 262 144

--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/batch_center_probe.py --only-batch --sets a --mods FSK)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = {"a": (4096, 16384), "lo": (512, 131072), "hi": (256, 262144)}
DISTINCT = 8                 # different captures per set, one per gain
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass


def captures(k, n, mod):
    import torch
    import noise_cases as nc
    base = []
    for s in range(min(DISTINCT, k)):
        sigma, amp = nc.STREAM_GAINS[s % len(nc.STREAM_GAINS)]
        base.append(torch.from_numpy(np.array(nc.capture(8000 + s, n, mod, sigma=sigma, amp=amp))).pin_memory())
    return [base[i % len(base)] for i in range(k)]


class Paths:
    def __init__(self, pipe, p, caps, n):
        import torch
        self.pipe, self.p, self.caps, self.n = pipe, p, caps, n
        self.np_caps = [c.numpy() for c in caps]
        self.stream = pipe.stream(n, p, want_qad=True, want_pos=False, auto_noise=True, auto_center=True)
        self.slots = [torch.empty((n, 2), dtype=torch.float32, device=pipe.device) for _ in range(4)]

    def a(self):
        return self.pipe.iq_to_bits_batch_center(self.np_caps, self.p, long_from=NEVER)

    def c(self):
        return self.pipe.iq_to_bits_batch_auto(self.np_caps, self.p, long_from=NEVER)

    def b(self, keep=None):
        n_out = 0

        def take(r):
            if keep is not None:
                keep[r.seq] = (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated), float(r.noise_threshold), int(r.noise_flag), r.center, int(r.center_flag))
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
            pp, bits, off, pauses, trunc, thr, flag, center, cflag = keep[seq0 + i]
            assert res.noise[i] == thr and res.noise_flags[i] == flag == 1, (i, res.noise[i], thr, flag)
            assert res.centers[i] == center and res.center_flags[i] == cflag, (i, res.centers[i], center, res.center_flags[i], cflag)
            if trunc or h.truncated:                         # (the two routes size their rows differently; a truncated result is not compared)
                n_trunc += 1
                continue
            assert np.array_equal(h.bits(), bits) and np.array_equal(h.ppseq(), pp) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
        flags = {f: res.center_flags.count(f) for f in (0, 1, 2, 3)}
        return sum(h.n_bits for h in res), n_trunc, flags, sorted({c for c in res.centers if c is not None})

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
    from urh_amd.batch import center, launch_counts
    dev = pipe.device
    paths = Paths(pipe, p, captures(k, n, p.modulation_type), n)
    n_bits, n_trunc, flags, centers = paths.verify()
    host = []
    settle = center._settle_centers                          # (looked up in urh_amd/batch/center.py by the function that calls it)

    def timed_settle(*a, **kw):                              # the host's share of one A: numpy on the tied histograms
        t0 = time.perf_counter()
        r = settle(*a, **kw)
        host.append((time.perf_counter() - t0) * 1e3)
        return r
    center._settle_centers = timed_settle
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
    center._settle_centers = settle
    host = host[-rounds:] or [0.0]
    ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
    line = (f"{p.modulation_type} {k:6d} x {n:8d}  A batch_center {fmt(a)} ms  B stream auto_noise+auto_center {fmt(b)} ms  C batch_auto {fmt(c)} ms  B/A {mb / ma:6.2f}  "
            f"A-C {ma - mc:8.2f} ms  host settling in A {statistics.median(host):8.2f} ms"
            f"  A: {k / ma * 1e3:10.0f} captures/s {k * n / ma * 1e3 / 1e9:7.3f} Gsamples/s  launches {after[0] - before[0]} copies {after[1] - before[1]}"
            f"  slowest A < fastest B: {max(a) < min(b)}  bits {n_bits}  truncated (not compared) {n_trunc}  center flags {flags}  centers {min(centers):.4g} .. {max(centers):.4g}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_center_probe.txt"))
    ap.add_argument("--mods", default="ASK,FSK")
    ap.add_argument("--sets", default="a,lo,hi")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    args = ap.parse_args()
    import torch
    import noise_cases as nc
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0, pipelined=True)
    mods = args.mods.split(",")
    if args.only_batch:
        for mod in mods:
            p = nc.params(mod, 1, write_pos=False)
            for s in args.sets.split(","):
                k, n = SETS[s]
                caps = [c.numpy() for c in captures(k, n, mod)]
                pipe.iq_to_bits_batch_center(caps, p, long_from=NEVER)
                ms = timed(lambda: pipe.iq_to_bits_batch_center(caps, p, long_from=NEVER), pipe.device)
                print(f"{mod} set ({s}) {k} x {n}: one batch with automatic noise thresholds and centers {ms:.2f} ms")
        return
    out = [f"# tools/batch_center_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); launches / copies: of one A",
           "# A = iq_to_bits_batch_center; B = pipelined CaptureStream(auto_noise=True, auto_center=True), push_upload per capture + flush; "
           "C = iq_to_bits_batch_auto: no center, not a lower bound (host arrays in, results on the host)"]
    for mod in mods:
        p = nc.params(mod, 1, write_pos=False)
        for s in args.sets.split(","):
            k, n = SETS[s]
            measure(pipe, p, k, n, args.rounds, out)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
