#!/usr/bin/env python3
"""tools/batch_each_probe.py [--out profiles/batch_each_probe.txt] [--sets 1,8,64,4096] [--rounds 5] [--limit 300]

A session whose captures have D different parameter sets, through the batch that takes a parameter set per capture and through what a user
did before it:

    A  ONE DevicePipeline.iq_to_bits_batch_each(captures, params, message_length_divisor=1)
    B  the captures grouped by equal parameters, DevicePipeline.iq_to_bits_batch_records(group, p, 1) per group: D batches
    C  (D = 1 only) iq_to_bits_batch_records with the one p: A - C is what the table costs

4096 captures of 16 384 float32 samples (tests/noise_cases.capture, four different ones per modulation), ASK and FSK mixed (D = 1: FSK
alone), RESIDENT ON THE DEVICE as one (iq_cat, starts); set j has its own center, tolerance and noise threshold.  One MI355X, one process per
D, the paths alternating: `rounds` rounds each after a warm-up, median (min - max).  Bits, offsets, pauses and records (RSSI by bit pattern) of
A and B are compared for equality before anything is timed.  Every D runs in a child process under its own time limit (--limit seconds), and
nothing is started after one that failed."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, N = 4096, 16384
NEVER = 1 << 40              # long_from of the timed batches: nothing is routed to a pass


def session(pipe, d):
    """(iq_cat on the device, starts, params per capture, set index per capture)"""
    import torch
    import noise_cases as nc
    from dataclasses import replace
    mods = ("FSK",) if d == 1 else ("ASK", "FSK")
    base = {m: [torch.from_numpy(np.array(nc.capture(8100 + s, N, m))).to(pipe.device) for s in range(4)] for m in mods}
    sets = []
    for j in range(d):
        m = mods[j % len(mods)]
        p = nc.params(m, 1, 0.1, write_pos=False)
        sets.append(replace(p, center=p.center + 1e-6 * j, tolerance=1 + j % 5, noise_threshold=0.1 + 1e-6 * j))
    which = [i % d for i in range(K)]
    cat = torch.cat([base[sets[j].modulation_type][i % 4] for i, j in enumerate(which)]).contiguous()
    return cat, np.arange(K + 1, dtype=np.int64) * N, sets, which


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def fmt(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} - {max(v):.2f})"


def snapshot(h):
    return h.bits(), h.msg_off.copy(), h.pauses.copy(), int(h.truncated), np.array(h.records)


def measure(d, rounds):
    import torch
    from urh_amd.batch import launch_counts
    from urh_amd.pipeline import DevicePipeline
    pipe = DevicePipeline(0)
    dev = pipe.device
    cat, starts, sets, which = session(pipe, d)
    params = [sets[j] for j in which]
    groups = [[i for i in range(K) if which[i] == j] for j in range(d)]
    views = [cat[i * N:(i + 1) * N] for i in range(K)]

    def a():
        return pipe.iq_to_bits_batch_each((cat, starts), params, message_length_divisor=1, long_from=NEVER)

    def b(keep=None):
        for j, idx in enumerate(groups):
            res = pipe.iq_to_bits_batch_records((cat, starts) if d == 1 else [views[i] for i in idx], sets[j], 1, long_from=NEVER)
            if keep is not None:
                for i, h in zip(idx, res):
                    keep[i] = snapshot(h)

    def c():
        return pipe.iq_to_bits_batch_records((cat, starts), sets[0], 1, long_from=NEVER)

    keep = {}
    b(keep)
    n_msg = n_trunc = 0
    for i, h in enumerate(a()):
        bits, off, pauses, trunc, rec = keep[i]
        assert h.truncated == trunc, i
        if trunc:
            n_trunc += 1
            continue
        mine = np.array(h.records)
        assert np.array_equal(h.bits(), bits) and np.array_equal(h.msg_off, off) and np.array_equal(h.pauses, pauses), i
        assert len(mine) == len(rec) and all(np.array_equal(mine[f], rec[f]) for f in ("first_pos", "mid_pos", "n_pad", "flag")), i
        assert np.array_equal(np.ascontiguousarray(mine["rssi"]).view(np.uint64), np.ascontiguousarray(rec["rssi"]).view(np.uint64)), i
        n_msg += len(mine)
    del keep
    paths = [a, b] + ([c] if d == 1 else [])
    for fn in paths:
        timed(fn, dev)
    t = [[] for _ in paths]
    for _ in range(rounds):
        before = launch_counts(pipe)
        t[0].append(timed(a, dev))
        after = launch_counts(pipe)
        for k in range(1, len(paths)):
            t[k].append(timed(paths[k], dev))
    ma, mb = statistics.median(t[0]), statistics.median(t[1])
    line = (f"D {d:5d}  {K} x {N} float32  A batch_each {fmt(t[0])} ms  B batch_records per group {fmt(t[1])} ms  B/A {mb / ma:8.2f}  "
            f"slowest A < fastest B: {max(t[0]) < min(t[1])}  A: launches {after[0] - before[0]} copies {after[1] - before[1]}  "
            f"messages {n_msg}  truncated (equal, not compared further) {n_trunc}")
    if d == 1:
        mc = statistics.median(t[2])
        line += f"  C batch_records {fmt(t[2])} ms  A - C {ma - mc:7.2f} ms  A median / C slowest {ma / max(t[2]):5.3f}"
    return f"# {torch.cuda.get_device_name(0)}, rounds {rounds}, median (min - max)\n" + line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_each_probe.txt"))
    ap.add_argument("--sets", default="1,8,64,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--one", type=int, default=0, help="(a child's part: this D alone, the line on standard output)")
    args = ap.parse_args()
    if args.one:
        print(measure(args.one, args.rounds), flush=True)
        return 0
    out = ["# tools/batch_each_probe.py: A = one iq_to_bits_batch_each (divisor 1); B = iq_to_bits_batch_records per group of equal parameters; "
           "C = iq_to_bits_batch_records with the one parameter set (D = 1); captures resident on the device, results on the host"]
    status = 0
    for d in args.sets.split(","):
        try:
            got = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", d, "--rounds", str(args.rounds)], capture_output=True, text=True,
                                 timeout=args.limit)
        except subprocess.TimeoutExpired:
            out.append(f"D {d}: not finished within {args.limit} s; nothing was started after it")
            status = 124
            break
        lines = [ln for ln in got.stdout.splitlines() if ln.startswith(("D ", "# "))]
        out += lines
        print("\n".join(lines), flush=True)
        if got.returncode != 0:
            out.append(f"D {d}: exit status {got.returncode}; nothing was started after it\n" + got.stderr[-2000:])
            status = got.returncode
            break
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
