#!/usr/bin/env python3
"""Automatic noise threshold inside a pass against the only route the library had to the same results: per-pass wall time.

PASSES captures (complex64 2-FSK bursts in noise, four distinct ones with different gains, cycled) of 2^20 and of 2^27 samples, results on
the host, warm-up first, then ROUNDS rounds in ONE process with the two sides alternating inside every round; ms per pass, median and
min - max over the rounds:
  queued  CaptureStream(auto_noise=True): push, push, ... flush -- the threshold is decided on the device, the host never waits in a push
  parent  capture after capture: estimators.detect_noise_level_dev (2 x n_chunks doubles come back: a host round trip), then
          pipe.iq_to_bits with that threshold, .host()
The thresholds of the two sides are compared; the margin a comparison has to respect is the parent side's own spread.

    python tools/auto_noise_probe.py [--out profiles/auto_noise_probe.txt] [--sizes 1048576,134217728] [--tag run1]
"""
import argparse
import os
import statistics
import sys
import time
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 5
PASSES = 20
GAINS = (1.0, 0.1, 0.5, 0.2)


def capture(torch, n, seed, gain, sps=100):
    """noise of sigma 0.01 with three 2-FSK bursts (+-20 kHz at 1 MS/s) of amplitude 0.5, times `gain`; the first and the last tenth silent"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bits = torch.randint(0, 2, (n // sps + 1,), generator=g, device="cuda")
    f = (bits.double() * 2 - 1).repeat_interleave(sps)[:n] * (2 * torch.pi * 20e3 / 1e6)
    ph = torch.cumsum(f, 0)
    iq = torch.stack([torch.cos(ph), torch.sin(ph)], 1).float() * 0.5
    del ph, f, bits
    lo, seg = n // 10, (n - 2 * (n // 10)) // 3
    k = torch.arange(n, device="cuda")
    on = (k >= lo) & (k < lo + 3 * seg) & (((k - lo) % seg) < (2 * seg) // 3)
    iq[~on] = 0
    del k, on
    iq += 0.01 * torch.randn((n, 2), generator=g, device="cuda")
    return (iq * gain).contiguous()


def spread(values):
    return f"{statistics.median(values):9.4f}  ({min(values):.4f} - {max(values):.4f})"


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "auto_noise_probe.txt"))
    ap.add_argument("--sizes", default="1048576,134217728")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import torch
    from urh_amd import estimators
    from urh_amd.pipeline import DemodParams, DevicePipeline

    def emit(s):
        """print and APPEND to --out: the runs of one comparison end up in one file, each under its own heading (--tag)"""
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(s + "\n")

    emit(f"auto_noise_probe {args.tag}: {torch.cuda.get_device_name(0)}, complex64 2-FSK, {PASSES} passes, ms per pass until the results are on the host, "
         f"median (min - max) of {ROUNDS} rounds, sides alternating in every round")
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, True)
    for n in (int(x) for x in args.sizes.split(",")):
        caps = [capture(torch, n, 7 + k, g) for k, g in enumerate(GAINS)]
        torch.cuda.synchronize()
        pipe = DevicePipeline(0)
        stream = pipe.stream(n, p, want_qad=True, want_pos=True, auto_noise=True)

        def queued():
            thr = []
            t0 = time.perf_counter()
            for k in range(PASSES):
                r = stream.push(caps[k % len(caps)])
                if r is not None:
                    thr.append(r.check().noise_threshold)
            thr += [r.check().noise_threshold for r in stream.flush()]
            return (time.perf_counter() - t0) * 1e3 / PASSES, thr

        def parent():
            thr = []
            t0 = time.perf_counter()
            for k in range(PASSES):
                iq = caps[k % len(caps)]
                t = estimators.detect_noise_level_dev(pipe, iq)
                pipe.iq_to_bits(iq, replace(p, noise_threshold=float(t)), want_qad=True).host().check()
                thr.append(float(t))
            return (time.perf_counter() - t0) * 1e3 / PASSES, thr

        for _ in range(2):
            queued(); parent()
        a, b = [], []
        for _ in range(ROUNDS):
            t, thr_new = queued(); a.append(t)
            t, thr_old = parent(); b.append(t)
        ratio = statistics.median(b) / statistics.median(a)
        emit(f"n = {n:>9}   queued {spread(a)}   parent {spread(b)}   parent / queued {ratio:.2f}   thresholds {sorted(set(thr_new))} "
             f"{'==' if thr_new == thr_old else '!='} parent's")
        stream.close()
        del caps, stream, pipe
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
