#!/usr/bin/env python3
"""Automatic center inside a pass against the sequence it replaces: wall time until the results are on the host.

For seeded captures of 10^5, 10^6 and 2^27 samples (complex64, 2-FSK at +-100 kHz with gated gaps; the same capture demodulated as ASK),
max_size 7500 and None, warm-up first, then ROUNDS rounds in ONE process with the two sides alternating inside every round; median and
min - max in ms:
  new     pipe.iq_to_bits(d, p, auto_center=True, center_max_size=m) -> .center, .host()
  parent  qad = pipe.afp_demod(d, p); c = estimators.detect_center_dev(pipe, qad, max_size=m); pipe.qad_to_bits(qad, p with c).host()
Run it three times (--tag run1 ...: every run appends to --out under its own heading); the margin a comparison has to respect is the
parent side's own spread across the runs.

    python tools/auto_center_probe.py [--out profiles/auto_center_probe.txt] [--sizes 100000,1000000,134217728] [--tag run1]
"""
import argparse
import os
import statistics
import sys
import time
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 7


def fsk_capture(torch, n, seed, sps=50):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bits = torch.randint(0, 2, (n // sps + 1,), generator=g, device="cuda")
    f = (bits.double() * 2 - 1).repeat_interleave(sps)[:n] * (2 * torch.pi * 100e3 / 1e6)
    ph = torch.cumsum(f, 0)
    iq = torch.stack([torch.cos(ph), torch.sin(ph)], 1).float()
    del ph, f
    k = torch.arange(n, device="cuda") % 3200
    iq[k >= 2500] = 0                                            # silent gaps: gated samples, the compaction path
    return (iq + 0.05 * torch.randn((n, 2), generator=g, device="cuda")).contiguous()


def spread(values):
    return f"{statistics.median(values):9.4f}  ({min(values):.4f} - {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "auto_center_probe.txt"))
    ap.add_argument("--sizes", default="100000,1000000,134217728")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import torch
    from urh_amd import estimators
    from urh_amd.pipeline import DemodParams, DevicePipeline
    lines = [f"auto_center_probe {args.tag}: {torch.cuda.get_device_name(0)}, complex64, ms until the results are on the host, median (min - max) of {ROUNDS} "
             "rounds, sides alternating in every round"]

    def emit(s):
        """print and APPEND to --out: the runs of one comparison end up in one file, each under its own heading (--tag)"""
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(s + "\n")

    emit(lines[0])

    pipe = DevicePipeline(0)
    for n in (int(x) for x in args.sizes.split(",")):
        iq = fsk_capture(torch, n, 7)
        torch.cuda.synchronize()
        cap_rows = n // 6 + 2 if n <= 10 ** 6 else None
        for mod in ("FSK", "ASK"):
            p = DemodParams(mod, 1, 0.3, 0.0 if mod == "FSK" else 0.25, 1.0, 5, 50, 0.1, 8, True)
            for m in (7500, None):
                def new():
                    t0 = time.perf_counter()
                    res = pipe.iq_to_bits(iq, p, want_qad=True, cap_rows=cap_rows, auto_center=True, center_max_size=m)
                    c = res.center
                    res.host().check()
                    return (time.perf_counter() - t0) * 1e3, c, res.center_flag

                def parent():
                    t0 = time.perf_counter()
                    qad = pipe.afp_demod(iq, p)
                    c = estimators.detect_center_dev(pipe, qad, max_size=m)
                    res = pipe.qad_to_bits(qad, replace(p, center=p.center if c is None else float(c)), cap_rows=cap_rows)
                    res.host().check()
                    return (time.perf_counter() - t0) * 1e3, c

                for _ in range(2):
                    new(); parent()
                a, b = [], []
                for _ in range(ROUNDS):
                    t, c_new, flag = new(); a.append(t)
                    t, c_old = parent(); b.append(t)
                same = (c_new is None and c_old is None) or (c_new is not None and c_old is not None and float(c_new) == float(c_old))
                emit(f"n = {n:>9}  {mod}  max_size {str(m):>5}   new {spread(a)}   parent {spread(b)}   flag {flag} center {c_new} {'==' if same else '!='} parent's")
        del iq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
