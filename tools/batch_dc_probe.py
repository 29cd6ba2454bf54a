#!/usr/bin/env python3
"""tools/batch_dc_probe.py [--out profiles/batch_dc_probe.txt] [--sets a,b,c,d,e] [--rounds 5]

A batch of captures with DC correction (DevicePipeline.iq_to_bits_batch_dc: two launches correct every capture on the device, then the
batch) against what a user wrote before it: a pipelined CaptureStream(dc_correction=True) with one upload, one correction and one pass per
capture.  One MI355X, one process, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: 2-FSK at 100
samples per symbol on a DC term from a seeded generator, pinned host arrays; results on the host for every path; the paths' bits and pulse
tables are compared before anything is timed.

    A   the stream: per capture an upload into a device slot, push() -- existing code
    B   iq_to_bits_batch_dc(host arrays)
    B0  iq_to_bits_batch(host arrays corrected beforehand, with numpy): B - B0 is what the two launches cost

    set (a) 4096 x 16 384 float32   (b) 4096 x 16 384 int16   (c) 512 x 131 072   (d) 341 x 196 608   (e) 256 x 262 144   (c - e: float32)

The table is read for B / A, for B - B0, and for the length at which a capture should leave the batch (urh_amd/batch/inputs.py LONG_FROM_DEFAULT;
DESIGN.md 7.7k)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"a": (4096, 16384, np.float32), "b": (4096, 16384, np.int16), "c": (512, 131072, np.float32), "d": (341, 196608, np.float32),
        "e": (256, 262144, np.float32)}
DISTINCT = 8                 # different captures per set (the rest repeat them: what is timed does not depend on the contents' variety)
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass


def fsk_on_dc(n, seed, dtype):
    """seeded 2-FSK at 100 samples per symbol, +-20 kHz at 1 MS/s, amplitude 0.5, AWGN, silent gaps, on the DC term (0.2, 0.1)"""
    rng = np.random.default_rng(seed)
    f = np.repeat(np.where(rng.integers(0, 2, n // 100 + 1) == 1, 20e3, -20e3), 100)[:n]
    ph = np.cumsum(2 * np.pi * f / 1e6)
    iq = 0.5 * np.stack([np.cos(ph), np.sin(ph)], 1)
    for a in range(3000, n, 4500):
        iq[a:a + 1500] = 0
    iq = iq + 0.01 * rng.standard_normal((n, 2)) + (0.2, 0.1)
    return iq.astype(np.float32) if np.dtype(dtype) == np.float32 else np.round(iq * 20_000).astype(dtype)


def numpy_dc(x):
    d = x - np.mean(x, axis=0)
    return d if x.dtype == np.float32 else d.astype(x.dtype)


class Paths:
    def __init__(self, pipe, p, k, n, dtype):
        import torch
        self.pipe, self.p, self.k = pipe, p, k
        base = [torch.from_numpy(fsk_on_dc(n, 4321 + s, dtype)).pin_memory() for s in range(min(DISTINCT, k))]     # pinned: PCIe speed for the uploads
        fixed = [numpy_dc(c.numpy()) for c in base]
        self.caps = [base[i % len(base)] for i in range(k)]
        self.np_caps = [c.numpy() for c in self.caps]
        self.np_fixed = [fixed[i % len(base)] for i in range(k)]
        self.stream = pipe.stream(n, p, want_qad=False, want_pos=False, dtype=dtype, dc_correction=True)
        self.slots = [torch.empty((n, 2), dtype=base[0].dtype, device=pipe.device) for _ in range(4)]     # a result is handed out three pushes later

    def batch_dc(self):
        return self.pipe.iq_to_bits_batch_dc(self.np_caps, self.p, long_from=NEVER)

    def batch_plain(self):
        return self.pipe.iq_to_bits_batch(self.np_fixed, self.p, long_from=NEVER)

    def stream_pass(self, keep=None):
        n_out = 0

        def note(r):
            if keep is not None:
                keep[r.seq] = (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated))
        for i, c in enumerate(self.caps):
            slot = self.slots[i % 4]
            slot.copy_(c, non_blocking=True)
            r = self.stream.push(slot)
            if r is not None:
                n_out += 1
                note(r)
        for r in self.stream.flush():
            n_out += 1
            note(r)
        assert n_out == self.k

    def verify(self):
        keep = {}
        self.stream_pass(keep)
        seq0 = min(keep)
        for res in (self.batch_dc(), self.batch_plain()):
            assert len(res) == self.k and res.truncated == [], res.truncated
            for i, h in enumerate(res):
                pp, bits, off, pauses, trunc = keep[seq0 + i]
                assert not trunc and len(pp) > 10
                assert np.array_equal(h.bits(), bits) and np.array_equal(h.ppseq(), pp) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
            n_bits = sum(h.n_bits for h in res)
        return n_bits

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


def measure(pipe, k, n, dtype, rounds, out):
    from urh_amd.batch import launch_counts
    from urh_amd.pipeline import DemodParams
    scale = 1.0 if np.dtype(dtype) == np.float32 else 20_000.0
    p = DemodParams("FSK", 1, 0.1 * scale, 0.0, 1.0, 5, 100, 0.1, 8, False)
    dev = pipe.device
    paths = Paths(pipe, p, k, n, dtype)
    n_bits = paths.verify()
    for fn in (paths.stream_pass, paths.batch_dc, paths.batch_plain):         # warm-up (buffers grown, pinned memory there)
        timed(fn, dev)
    a, b, b0, launches = [], [], [], []
    for _ in range(rounds):
        a.append(timed(paths.stream_pass, dev))
        l0 = launch_counts(pipe)[0]
        b.append(timed(paths.batch_dc, dev))
        l1 = launch_counts(pipe)[0]
        b0.append(timed(paths.batch_plain, dev))
        launches.append((l1 - l0, launch_counts(pipe)[0] - l1))
    paths.close()
    ma, mb, mb0 = (statistics.median(v) for v in (a, b, b0))
    line = (f"{k:6d} x {n:8d} {np.dtype(dtype).name:8s} A stream {fmt(a)} ms  B batch_dc {fmt(b)} ms  B0 batch {fmt(b0)} ms  B/A {mb / ma:6.3f}  B-B0 {mb - mb0:8.3f} ms"
            f"  launches B {launches[-1][0]} B0 {launches[-1][1]}  slowest B < fastest A: {max(b) < min(a)}  bits {n_bits}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_dc_probe.txt"))
    ap.add_argument("--sets", default="a,b,c,d,e")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0, pipelined=True)
    out = [f"# tools/batch_dc_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max)",
           "# A = pipelined CaptureStream(dc_correction=True): upload + push per capture, flush; B = iq_to_bits_batch_dc (host arrays in, results on the host);",
           "# B0 = iq_to_bits_batch on the same captures corrected beforehand with numpy"]
    for s in args.sets.split(","):
        k, n, dtype = SETS[s]
        measure(pipe, k, n, dtype, args.rounds, out)
        with open(args.out, "w") as fh:                    # (after every set: a run that is cut short keeps what it has measured)
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
