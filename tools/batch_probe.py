#!/usr/bin/env python3
"""tools/batch_probe.py [--out profiles/batch_probe.txt] [--sets a,b,c] [--rounds 5] [--search 3]

A batch of captures (DevicePipeline.iq_to_bits_batch: a wavefront per capture, three launches) against what a user wrote before it: a
pipelined CaptureStream with one pass per capture (push_upload, flush).  One MI355X, one process, the two paths alternating: `rounds`
rounds each after a warm-up, median (min - max).  Captures: float32 2-FSK at 100 samples per symbol (urh_amd.synth.fsk_capture), host
arrays; results on the host for both paths; both paths' bits and pulse tables are compared before anything is timed.

    set (a)  4096 captures of 16 384 samples      set (b)  512 of 262 144      set (c)  64 of 2^21

--search N: N more lengths by halving (in log2) between the two neighbouring lengths that straddle B / A = 1: the crossover, which is
DevicePipeline.iq_to_bits_batch's default `long_from` (urh_amd/batch/inputs.py LONG_FROM_DEFAULT).
--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/batch_probe.py
--only-batch --sets a)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"a": (4096, 16384), "b": (512, 262144), "c": (64, 1 << 21)}
DISTINCT = 8                 # different captures per set (the rest repeat them: what is timed does not depend on the contents' variety)
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass


def captures(k, n, dev):
    import torch
    from urh_amd.synth import fsk_capture
    base = []
    for s in range(min(DISTINCT, k)):
        iq, _ = fsk_capture(1, dev, seed=4321 + s, seg_len=n)
        base.append(iq.cpu().pin_memory())           # pinned: PCIe speed for the stream's uploads (the batch packs into its own pinned buffer)
    torch.cuda.synchronize(dev)
    return [base[i % len(base)] for i in range(k)]


class Paths:
    def __init__(self, pipe, p, caps, n):
        import torch
        self.pipe, self.p, self.caps, self.n = pipe, p, caps, n
        self.np_caps = [c.numpy() for c in caps]
        self.stream = pipe.stream(n, p, want_qad=False, want_pos=False)
        self.slots = [torch.empty((n, 2), dtype=torch.float32, device=pipe.device) for _ in range(4)]     # a result is handed out three pushes later

    def batch(self):
        return self.pipe.iq_to_bits_batch(self.np_caps, self.p, long_from=NEVER)

    def stream_pass(self, keep=None):
        n_out = 0
        for i, c in enumerate(self.caps):
            r = self.stream.push_upload(c, self.slots[i % 4])
            if r is not None:
                n_out += 1
                if keep is not None:
                    keep[r.seq] = (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated))
        for r in self.stream.flush():
            n_out += 1
            if keep is not None:
                keep[r.seq] = (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated))
        assert n_out == len(self.caps)

    def verify(self):
        keep = {}
        self.stream_pass(keep)
        seq0 = min(keep)
        res = self.batch()
        assert len(res) == len(self.caps) and res.truncated == [], res.truncated
        for i, h in enumerate(res):
            pp, bits, off, pauses, trunc = keep[seq0 + i]
            assert not trunc
            assert np.array_equal(h.bits(), bits) and np.array_equal(h.ppseq(), pp) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
        return sum(h.n_bits for h in res)

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
    paths = Paths(pipe, p, captures(k, n, dev), n)
    n_bits = paths.verify()
    timed(paths.batch, dev); timed(paths.stream_pass, dev)                    # warm-up (buffers grown, pinned memory there)
    a, b = [], []
    before = launch_counts(pipe)
    for _ in range(rounds):
        a.append(timed(paths.batch, dev))
        b.append(timed(paths.stream_pass, dev))
    after = launch_counts(pipe)
    paths.close()
    ma, mb = statistics.median(a), statistics.median(b)
    line = (f"{k:6d} x {n:8d}  batch {fmt(a)} ms  stream {fmt(b)} ms  B/A {mb / ma:6.2f}  batch: {k / ma * 1e3:10.0f} captures/s {k * n / ma * 1e3 / 1e9:7.3f} Gsamples/s"
            f"  stream: {k / mb * 1e3:9.0f} captures/s {k * n / mb * 1e3 / 1e9:7.3f} Gsamples/s  launches {(after[0] - before[0]) // rounds} copies {(after[1] - before[1]) // rounds + 1}"
            f"  slowest batch < fastest stream: {max(a) < min(b)}  bits {n_bits}")
    print(line, flush=True)
    out.append(line)
    return mb / ma, max(a) < min(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_probe.txt"))
    ap.add_argument("--sets", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--search", type=int, default=3)
    ap.add_argument("--only-batch", action="store_true")
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    pipe = DevicePipeline(0, pipelined=True)
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
    if args.only_batch:
        for s in args.sets.split(","):
            k, n = SETS[s]
            caps = [c.numpy() for c in captures(k, n, pipe.device)]
            pipe.iq_to_bits_batch(caps, p, long_from=NEVER)
            ms = timed(lambda: pipe.iq_to_bits_batch(caps, p, long_from=NEVER), pipe.device)
            print(f"set ({s}) {k} x {n}: one batch {ms:.2f} ms")
        return
    out = [f"# tools/batch_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); copies: the upload + the directory + the blob",
           "# path A = iq_to_bits_batch (host arrays in, results on the host); path B = pipelined CaptureStream, push_upload per capture + flush"]
    ratios = {}
    for s in args.sets.split(","):
        k, n = SETS[s]
        ratios[n] = measure(pipe, p, k, n, args.rounds, out)
    if args.search > 0 and len(ratios) > 1:
        total = 1 << 26
        for _ in range(args.search):
            ns = sorted(ratios)
            pair = [(x, y) for x, y in zip(ns[:-1], ns[1:]) if ratios[x][0] >= 1.0 > ratios[y][0]]
            if not pair:
                break
            lo, hi = pair[0]
            mid = 1 << ((lo.bit_length() + hi.bit_length() - 2) // 2)
            if mid in ratios or mid <= lo or mid >= hi:
                mid = (lo + hi) // 2 // 1024 * 1024
                if mid in ratios or mid <= lo:
                    break
            ratios[mid] = measure(pipe, p, max(total // mid, 8), mid, args.rounds, out)
        ns = sorted(ratios)
        wins = [x for x in ns if ratios[x][0] >= 1.0]
        loses = [x for x in ns if ratios[x][0] < 1.0]
        line = f"# batch at least as fast up to {max(wins) if wins else None} samples per capture, stream faster from {min(loses) if loses else None}: long_from"
        print(line)
        out.append(line)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
