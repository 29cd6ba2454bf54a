#!/usr/bin/env python3
"""tools/batch_records_probe.py [--out profiles/batch_records_probe.txt] [--sets a,lo] [--mods ASK,FSK] [--rounds 5]

A batch of captures that ends with its message records (DevicePipeline.iq_to_bits_batch_records) against the fastest route to the same
records before it, and against the batch without records:

    A  iq_to_bits_batch_records (message_length_divisor 8)
    B  a pipelined CaptureStream(msg_records=True, message_length_divisor=8), push_upload per capture + flush
    C  iq_to_bits_batch: the same walk without the records; what the records cost is A - C

One MI355X, one process, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Captures: float32 ASK and
2-FSK bursts with quiet chunks (tests/noise_cases.capture), eight different ones per set, pinned host arrays, one configured noise
threshold.  The records (RSSI by bit pattern), bits and pauses of A and B are compared before anything is timed.

    set (a)   4096 captures of 16 384 samples      set (lo)  512 of 131 072

--only-batch: path A alone, once per set after a warm-up (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/batch_records_probe.py --only-batch --sets a --mods FSK)."""
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
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass
DIVISOR = 8
NOISE = 0.1                  # between the noise floor (sigma 0.01) and the bursts (amplitude 0.5) of noise_cases.capture


def captures(k, n, mod):
    import torch
    import noise_cases as nc
    base = [torch.from_numpy(np.array(nc.capture(8100 + s, n, mod))).pin_memory() for s in range(min(DISTINCT, k))]
    return [base[i % len(base)] for i in range(k)]


class Paths:
    def __init__(self, pipe, p, caps, n):
        import torch
        self.pipe, self.p, self.caps, self.n = pipe, p, caps, n
        self.np_caps = [c.numpy() for c in caps]
        self.stream = pipe.stream(n, p, want_qad=True, want_pos=False, msg_records=True, message_length_divisor=DIVISOR)
        self.slots = [torch.empty((n, 2), dtype=torch.float32, device=pipe.device) for _ in range(4)]

    def a(self):
        return self.pipe.iq_to_bits_batch_records(self.np_caps, self.p, DIVISOR, long_from=NEVER)

    def c(self):
        return self.pipe.iq_to_bits_batch(self.np_caps, self.p, long_from=NEVER)

    def b(self, keep=None):
        n_out = 0

        def take(r):
            if keep is not None:
                keep[r.seq] = (r.bits(), r.msg_off.copy(), r.pauses.copy(), int(r.truncated), np.array(r.records))
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
        n_trunc = n_msg = 0
        for i, h in enumerate(res):
            bits, off, pauses, trunc, rec = keep[seq0 + i]
            if trunc or h.truncated:                         # (the two routes size their rows differently; a truncated result is not compared)
                n_trunc += 1
                continue
            assert np.array_equal(h.bits(), bits) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
            mine = np.array(h.records)
            assert len(mine) == len(rec) and (mine["flag"] == 1).all(), i
            for f in ("first_pos", "mid_pos", "n_pad", "flag"):
                assert np.array_equal(mine[f], rec[f]), (i, f)
            assert np.array_equal(np.ascontiguousarray(mine["rssi"]).view(np.uint64), np.ascontiguousarray(rec["rssi"]).view(np.uint64)), i
            n_msg += len(mine)
        return n_msg, n_trunc


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
    paths = Paths(pipe, p, captures(k, n, p.modulation_type), n)
    n_msg, n_trunc = paths.verify()
    for fn in (paths.a, paths.b, paths.c):                   # warm-up (buffers grown, pinned memory there)
        timed(fn, dev)
    a, b, c = [], [], []
    for _ in range(rounds):
        before = launch_counts(pipe)
        a.append(timed(paths.a, dev))
        after = launch_counts(pipe)
        b.append(timed(paths.b, dev))
        c.append(timed(paths.c, dev))
    paths.stream.close()
    ma, mb, mc = statistics.median(a), statistics.median(b), statistics.median(c)
    line = (f"{p.modulation_type} {k:6d} x {n:8d}  A batch_records {fmt(a)} ms  B stream msg_records {fmt(b)} ms  C batch {fmt(c)} ms  B/A {mb / ma:6.2f}  "
            f"A-C {ma - mc:8.2f} ms  A: {k / ma * 1e3:10.0f} captures/s {k * n / ma * 1e3 / 1e9:7.3f} Gsamples/s  launches {after[0] - before[0]} copies "
            f"{after[1] - before[1]}  slowest A < fastest B: {max(a) < min(b)}  messages {n_msg}  truncated (not compared) {n_trunc}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_records_probe.txt"))
    ap.add_argument("--mods", default="ASK,FSK")
    ap.add_argument("--sets", default="a,lo")
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
            p = nc.params(mod, 1, NOISE, write_pos=False)
            for s in args.sets.split(","):
                k, n = SETS[s]
                caps = [c.numpy() for c in captures(k, n, mod)]
                pipe.iq_to_bits_batch_records(caps, p, DIVISOR, long_from=NEVER)
                ms = timed(lambda: pipe.iq_to_bits_batch_records(caps, p, DIVISOR, long_from=NEVER), pipe.device)
                print(f"{mod} set ({s}) {k} x {n}: one batch with message records {ms:.2f} ms")
        return
    out = [f"# tools/batch_records_probe.py: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, median (min - max); launches / copies: of one A",
           f"# A = iq_to_bits_batch_records (divisor {DIVISOR}); B = pipelined CaptureStream(msg_records=True), push_upload per capture + flush; "
           "C = iq_to_bits_batch, the same walk without records (host arrays in, results on the host)"]
    for mod in mods:
        p = nc.params(mod, 1, NOISE, write_pos=False)
        for s in args.sets.split(","):
            k, n = SETS[s]
            measure(pipe, p, k, n, args.rounds, out)
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
