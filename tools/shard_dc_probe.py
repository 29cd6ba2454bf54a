#!/usr/bin/env python3
"""ShardedPipeline.dc_correct ("DC correction across the shards") on the bench's float32 FSK capture of 2^27 samples, run as
8 ranks -- threads on the one GPU, one GpuShardEngine each, ThreadComm -- beside urhgpu_dc_correct_dev on the whole capture.

Two captures: the bench's own (zero mean: the running sum wanders through zero and across binades) and the same on a DC term of 0.3 (what the
correction is for).  Per capture: the single-GPU call's time, then per rank the time of dc_correct (a host clock around the call in the rank's
thread, the GPU drained before and after; the ranks' kernels share the one GPU and every exchange is a barrier of the threads plus device
synchronisations, so a rank's time contains its wait for the others), the all-gather count and the rank's stitch statistics.  The stitched
result is compared with the single-GPU one bit for bit.  Median and min - max of ROUNDS rounds after one warm-up round.

    python tools/shard_dc_probe.py [--log2n 27] [--world 8] [--out profiles/shard_dc_probe.txt]
"""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5


def spread(values):
    return f"{statistics.median(values):9.3f}  ({min(values):.3f} - {max(values):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_dc_probe.txt"))
    args = ap.parse_args()
    import torch
    from urh_amd.filter import dc_correct_dev
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm, shard_bounds
    from urh_amd.synth import fsk_capture
    n, world = 1 << args.log2n, args.world
    pipe = DevicePipeline(0)
    dev = pipe.device
    engines = [GpuShardEngine(0) for _ in range(world)]
    bounds = shard_bounds(n, world)
    lines = [f"shard_dc_probe: float32 FSK capture of {n} samples ({n * 8 / 2 ** 30:.2f} GiB), {world} ranks as threads on one GPU; ms, median (min - max) of "
             f"{ROUNDS} rounds after one warm-up round"]
    print(lines[0], flush=True)
    iq, _ = fsk_capture(max(1, n >> 20), dev, seed=1234)
    iq = iq[:n]
    status = 0
    for name, offset in (("bench capture (zero mean)", 0.0), ("bench capture + 0.3", 0.3)):
        x = (iq + offset).contiguous() if offset else iq
        want = torch.empty_like(x)
        ms = []
        for k in range(ROUNDS + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, mean = dc_correct_dev(pipe, x, out=want, want_mean=True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"{name}: urhgpu_dc_correct_dev on the whole capture: {spread(ms[1:])}   mean {mean.cpu().numpy()}")
        print(lines[-1], flush=True)
        shared = ThreadComm.Shared(world)
        times, last, outs, errs = [[] for _ in range(world)], [None] * world, [None] * world, []

        def work(r):
            try:
                sp = ShardedPipeline(engines[r], ThreadComm(shared, r))
                a, b = bounds[r]
                for k in range(ROUNDS + 1):
                    torch.cuda.synchronize()
                    shared.barrier.wait()
                    t0 = time.perf_counter()
                    outs[r] = sp.dc_correct(x[a:b], pos_base=a, n_total=n)
                    torch.cuda.synchronize()
                    if k:
                        times[r].append((time.perf_counter() - t0) * 1e3)
                last[r] = sp.last_dc
            except BaseException as exc:            # noqa: BLE001 -- reported below
                errs.append((r, exc))
                shared.barrier.abort()
        ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(600)
        if errs or any(t.is_alive() for t in ts):
            lines.append(f"{name}: FAILED: {errs or 'a rank hangs'}")
            print(lines[-1], flush=True)
            status = 1
            break
        same = all(torch.equal(outs[r].view(torch.int32), want[a:b].view(torch.int32)) for r, (a, b) in enumerate(bounds))
        lines.append(f"{name}: sharded, all-gathers {last[0]['all_gathers']} (bound {world + 1}), mean {last[0]['mean']}, equal to the single-GPU result bit for bit: {same}")
        for r in range(world):
            d = last[r]
            lines.append(f"    rank {r}: dc_correct {spread(times[r])}   chunks per column {d['chunks']}, derived {d['derived']}, re-evaluated {d['reevaluated']}")
        print("\n".join(lines[-world - 1:]), flush=True)
        if not same:
            status = 1
            break
        del outs, want
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
