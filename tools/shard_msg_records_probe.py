#!/usr/bin/env python3
"""ShardedPipeline.message_records beside the pass it follows: 2^20 float32 samples per rank (FSK bursts between silent gaps, 50 samples
per symbol), for one rank and for 8 ranks as threads on the one GPU over ThreadComm.  Per round every rank times, with a host clock and
the device drained before and after, (a) iq_to_bits and (b) message_records on the same shard and result; reported are the median and
min .. max over --rounds rounds of the slowest rank's time, and how many all-gathers and exchanged windows each run of the records took.
There is no threshold: the number to set the records beside is the pass's own time per rank from the same run.  With 8 ranks as
threads the ranks' kernels share the GPU and every all-gather is a barrier of Python threads: those figures bound the protocol's host
cost from above, they are not what 8 GPUs would take.  Appends one JSON line per world size to --out.

    python tools/shard_msg_records_probe.py [--log2n 20] [--rounds 5] [--warmup 2] [--out profiles/shard_msg_records_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def capture(n, torch, dev):
    """seeded 2-FSK at 50 samples per symbol, a silent gap of 1500 samples every 12 000, a little noise (made on the device)"""
    g = torch.Generator(device=dev).manual_seed(3)
    sym = torch.randint(0, 2, (n // 50 + 1,), generator=g, device=dev).repeat_interleave(50)[:n]
    phase = torch.cumsum(torch.where(sym == 1, 0.1257, -0.1257).to(torch.float64), 0)
    amp = torch.where(torch.arange(n, device=dev) % 12_000 < 10_500, 1.0, 0.0).to(torch.float64)
    iq = torch.stack([torch.cos(phase) * amp, torch.sin(phase) * amp], 1).to(torch.float32)
    return iq + 0.02 * torch.randn((n, 2), generator=g, device=dev, dtype=torch.float32)


def run(world, n_rank, rounds, warmup):
    import torch
    from urh_amd.pipeline import DemodParams
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    dev = torch.device("cuda", 0)
    n = world * n_rank
    iq = capture(n, torch, dev)
    p = DemodParams("FSK", 1, 0.1, 0.0, 1.0, 5, 50, 0.1, 8, True)
    shared = ThreadComm.Shared(world)
    times = [[None] * world for _ in range(2)]
    info, err = [None] * world, []

    def work(r):
        try:
            sp = ShardedPipeline(GpuShardEngine(0), ThreadComm(shared, r))
            shard = iq[r * n_rank:(r + 1) * n_rank]
            t_pass, t_rec = [], []
            for it in range(warmup + rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = sp.iq_to_bits(shard, p, want_qad=False, pos_base=r * n_rank, n_total=n)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                rec = sp.message_records(shard, res, p, 1, pos_base=r * n_rank, n_total=n)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it >= warmup:
                    t_pass.append((t1 - t0) * 1e3)
                    t_rec.append((t2 - t1) * 1e3)
            times[0][r], times[1][r] = t_pass, t_rec
            info[r] = dict(sp.last_records, records=len(rec), valid=bool((rec["flag"] == 1).all()))
        except BaseException as e:          # noqa: BLE001 -- reported below
            err.append(e)
            shared.barrier.abort()
    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    if err or any(t.is_alive() for t in ts):
        raise RuntimeError(f"world {world}: {err or 'a rank hangs'}")

    def stats(per_rank):
        slowest = [max(per_rank[r][k] for r in range(world)) for k in range(rounds)]
        return {"ms_median": round(statistics.median(slowest), 3), "ms_min": round(min(slowest), 3), "ms_max": round(max(slowest), 3)}
    return {"world": world, "samples_per_rank": n_rank, "rounds": rounds, "pass": stats(times[0]), "message_records": stats(times[1]),
            "all_gathers": info[0]["all_gathers"], "windows_exchanged": info[0]["windows"], "records": sum(i["records"] for i in info),
            "all_valid": all(i["valid"] for i in info)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_msg_records_probe.txt"))
    args = ap.parse_args()
    import torch
    lines = []
    for world in (1, 8):
        line = dict(run(world, 1 << args.log2n, args.rounds, args.warmup), device=torch.cuda.get_device_name(0), clock="host, device drained")
        print(json.dumps(line), flush=True)
        lines.append(line)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
