#!/usr/bin/env python3
"""ShardedPipeline.iq_to_bits_auto(auto_center=True) against the two-pass recipe it replaces for ASK / FSK -- a pass with want_qad=True,
detect_center(result.qad), a second pass with that center -- on a 1-rank group (ThreadComm) over one float32 FSK capture of 2^log2n
samples (bursts between silent gaps, 50 samples per symbol, made on the device).  Both sides alternate in one process; per round each is
timed with a host clock, the device drained before and after and the result's counts read; reported are the median and min .. max over
--rounds rounds after --warmup warm-up rounds, and that both give the same center and the same counts.  There is no threshold: the
acceptance bar of the route is bit-exactness (tests/test_shard_auto_gpu.py).  Appends one JSON line to --out.

    python tools/shard_auto_probe.py [--log2n 27] [--rounds 7] [--warmup 2] [--out profiles/shard_auto_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def capture(n, torch, dev):
    """seeded 2-FSK at 50 samples per symbol, +-0.1 cycles per sample, a silent gap of 1500 samples every 12 000, a little noise: one block
    of 2^20 samples made on the device and repeated (the phase jumps at the block seams: one more symbol edge each)"""
    m = min(n, 1 << 20)
    g = torch.Generator(device=dev).manual_seed(3)
    sym = torch.randint(0, 2, (m // 50 + 1,), generator=g, device=dev).repeat_interleave(50)[:m]
    phase = torch.cumsum(torch.where(sym == 1, 0.6283, -0.6283).to(torch.float64), 0)
    amp = torch.where(torch.arange(m, device=dev) % 12_000 < 10_500, 1.0, 0.0).to(torch.float64)
    iq = torch.stack([torch.cos(phase) * amp, torch.sin(phase) * amp], 1).to(torch.float32)
    iq = iq + 0.02 * torch.randn((m, 2), generator=g, device=dev, dtype=torch.float32)
    return iq.repeat(n // m, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_auto_probe.txt"))
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DemodParams
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    iq = capture(n, torch, dev)
    p = DemodParams("FSK", 1, 0.1, 0.3, 1.0, 5, 50, 0.1, 8, True)
    sp = ShardedPipeline(GpuShardEngine(0), ThreadComm(ThreadComm.Shared(1), 0))

    def auto():
        res = sp.iq_to_bits_auto(iq, p, auto_center=True)
        return sp.last_center, res.host_counts()

    def recipe():
        first = sp.iq_to_bits(iq, p, want_qad=True)
        center = sp.detect_center(first.qad)
        res = sp.iq_to_bits(iq, p if center is None else replace(p, center=float(center)), want_qad=True)
        return (p.center if center is None else float(center)), res.host_counts()

    t = {"auto": [], "recipe": []}
    seen = {}
    for it in range(args.warmup + args.rounds):
        for name, fn in (("auto", auto), ("recipe", recipe)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seen[name] = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                t[name].append((time.perf_counter() - t0) * 1e3)

    def stats(v):
        return {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3)}
    line = {"samples": n, "rounds": args.rounds, "iq_to_bits_auto(auto_center)": stats(t["auto"]), "two_pass_recipe": stats(t["recipe"]),
            "center": seen["auto"][0], "same_center_and_counts": seen["auto"] == seen["recipe"], "all_gathers": sp.last_auto["all_gathers"],
            "device": torch.cuda.get_device_name(0), "clock": "host, device drained"}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
