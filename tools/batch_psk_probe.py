#!/usr/bin/env python3
"""tools/batch_psk_probe.py [--out profiles/batch_psk_probe.txt] [--sets a,b,c,d,e] [--rounds 5]

A batch of PSK captures (DevicePipeline.iq_to_bits_batch_psk: a Costas loop per capture in one launch, a lane per capture) against what a
user wrote before it: a pipelined CaptureStream of PSK captures with one pass per capture (push_upload, flush).  One MI355X, one process,
the two paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: float32 4-PSK at 100 samples per symbol
from a seeded generator (carrier offset, AWGN, a gated gap), pinned host arrays; results on the host for both paths; both paths' bits and
pulse tables are compared before anything is timed.

    set (a) 4096 x 8192    (b) 4096 x 16 384    (c) 1024 x 65 536    (d) 341 x 196 608    (e) a small session: 64 x 16 384

A's cost follows the LONGEST capture (the loop is serial, about 0.4 us per sample), B's the NUMBER of captures: the table is read for the
length at which a PSK capture should leave the batch (urh_amd/batch/inputs.py LONG_FROM_DEFAULT).
--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/batch_psk_probe.py --only-batch --sets a)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = {"a": (4096, 8192), "b": (4096, 16384), "c": (1024, 65536), "d": (341, 196608), "e": (64, 16384)}
DISTINCT = 8                 # different captures per set (the rest repeat them: what is timed does not depend on the contents' variety)
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass
NOISE = 0.2


def psk4(n, seed):
    """seeded 4-PSK at 100 samples per symbol: carrier offset 0.04 cycles per sample, AWGN, a gap at 1 % amplitude (gated: it freezes the loop)"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, n // 100 + 1)
    ph = np.repeat(np.array([-135, -45, 45, 135])[sym] * np.pi / 180, 100)[:n] + 2 * np.pi * 0.04 * np.arange(n)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1) + 0.1 * np.sqrt(0.5) * rng.standard_normal((n, 2))
    iq[n // 3:n // 3 + n // 7] *= 0.01
    return iq.astype(np.float32)


def captures(k, n):
    import torch
    base = [torch.from_numpy(psk4(n, 4321 + s)).pin_memory() for s in range(min(DISTINCT, k))]   # pinned: PCIe speed for the stream's uploads
    return [base[i % len(base)] for i in range(k)]


class Paths:
    def __init__(self, pipe, p, caps, n):
        import torch
        self.pipe, self.p, self.caps, self.n = pipe, p, caps, n
        self.np_caps = [c.numpy() for c in caps]
        self.stream = pipe.stream(n, p, want_qad=False, want_pos=False)
        self.slots = [torch.empty((n, 2), dtype=torch.float32, device=pipe.device) for _ in range(4)]     # a result is handed out three pushes later

    def batch(self):
        return self.pipe.iq_to_bits_batch_psk(self.np_caps, self.p, long_from=NEVER)

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
    paths = Paths(pipe, p, captures(k, n), n)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_psk_probe.txt"))
    ap.add_argument("--sets", default="a,b,c,d,e")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    pipe = DevicePipeline(0, pipelined=True)
    p = DemodParams("PSK", 2, NOISE, 0.0, 1.5, 5, 100, 0.1, 8, False)
    if args.only_batch:
        for s in args.sets.split(","):
            k, n = SETS[s]
            caps = [c.numpy() for c in captures(k, n)]
            pipe.iq_to_bits_batch_psk(caps, p, long_from=NEVER)
            ms = timed(lambda: pipe.iq_to_bits_batch_psk(caps, p, long_from=NEVER), pipe.device)
            print(f"set ({s}) {k} x {n}: one batch {ms:.2f} ms")
        return
    out = [f"# tools/batch_psk_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); copies: the upload + the directory + the blob",
           "# path A = iq_to_bits_batch_psk (host arrays in, results on the host); path B = pipelined CaptureStream of PSK captures, push_upload per capture + flush"]
    for s in args.sets.split(","):
        k, n = SETS[s]
        measure(pipe, p, k, n, args.rounds, out)
        with open(args.out, "w") as fh:                    # (after every set: a run that is cut short keeps what it has measured)
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
