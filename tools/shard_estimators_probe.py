#!/usr/bin/env python3
"""The sharded estimators (ShardedPipeline.detect_center / detect_noise_level) against the single-GPU functions on 2^27 samples:

    center    detect_center on a two-level demodulated signal with runs of -4:
                  sharded, one rank over ThreadComm | detect_center_dev(_single=True) | detect_center_dev (the batched pass),
                  alternating, and the sharded pass's phases (one extra pass, every engine call bracketed by a device synchronise)
    noise     detect_noise_level on a float32 capture with bursts of carrier: sharded, one rank | detect_noise_level_dev
    rccl1     both sharded calls over a 1-rank RcclComm (a process group of one rank; skipped where RCCL cannot be had)
    threads8  8 ranks as threads on the one GPU: equality with the single-GPU values only (the ranks' kernels share the GPU)

Without --step the script starts every step as a child process of its own under its own time limit and stops at the first that
fails; the record is the steps' JSON lines.  Times: a host clock around a call that ends with its result on the host (every call
does: the estimate is a Python float), the GPU drained before; --warmup calls first, the median of --reps.

    python tools/shard_estimators_probe.py [--log2n 27] [--reps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("center", 300), ("noise", 300), ("rccl1", 300), ("threads8", 420))


def demodulated(n, torch, dev):
    """two levels + a little noise; a run of -4 of 1 .. 1500 samples about every 3000 samples (seeded, made on the device)"""
    g = torch.Generator(device=dev).manual_seed(7)
    sym = torch.randint(0, 2, (n // 50 + 1,), generator=g, device=dev).repeat_interleave(50)[:n]
    x = torch.where(sym == 1, 0.8, -0.6).to(torch.float32) + 0.05 * torch.randn(n, generator=g, device=dev, dtype=torch.float32)
    blocks = n // 3000
    start = torch.arange(blocks, device=dev) * 3000 + torch.randint(0, 1500, (blocks,), generator=g, device=dev)
    length = torch.randint(1, 1500, (blocks,), generator=g, device=dev)
    pos = torch.arange(n, device=dev)
    b = torch.clamp(pos // 3000, max=blocks - 1)
    x[(pos >= start[b]) & (pos < start[b] + length[b])] = -4.0
    return x


def capture(n, torch, dev):
    """float32 IQ: noise at 2 % amplitude with bursts of carrier over a third of the capture"""
    g = torch.Generator(device=dev).manual_seed(11)
    amp = torch.where((torch.arange(n, device=dev) // max(1, n // 7)) % 3 == 1, 1.0, 0.02).to(torch.float32)
    return (torch.randn((n, 2), generator=g, device=dev, dtype=torch.float32) * 0.5 + 1.0) * amp[:, None]


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def alternating(torch, fns, warmup, reps):
    """{name: times}: the candidates warmed up, then timed in turn, `reps` rounds"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k] += timed(torch, fn, 0, 1)
    return out


def summary(times):
    return {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def phases(torch, engine, call):
    """one pass with every engine call bracketed by a device synchronise: ms per engine method, and the rest (exchanges + host)"""
    spent = {}
    names = ("compact_gt", "pairwise_partial", "histogram", "noise_partials")
    saved = {k: getattr(engine, k) for k in names}

    def wrap(name):
        f = saved[name]

        def g(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f(*a, **k)
            torch.cuda.synchronize()
            spent[name] = spent.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
            return r
        return g
    for k in names:
        setattr(engine, k, wrap(k))
    try:
        total = timed(torch, call, 0, 1)[0]
    finally:
        for k in names:
            delattr(engine, k)
    spent = {k: round(v, 3) for k, v in spent.items()}
    spent["exchanges_and_host"] = round(total - sum(spent.values()), 3)
    return spent


def step_center(args, torch, dev):
    from urh_amd.estimators import detect_center_dev
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    n = 1 << args.log2n
    x = demodulated(n, torch, dev)
    pipe, eng = DevicePipeline(0), GpuShardEngine(0)
    sp = ShardedPipeline(eng, ThreadComm(ThreadComm.Shared(1), 0))
    fns = {"sharded_rank1_threadcomm": lambda: sp.detect_center(x), "single": lambda: detect_center_dev(pipe, x, _single=True),
           "batched": lambda: detect_center_dev(pipe, x)}
    values = {k: fn() for k, fn in fns.items()}
    times = alternating(torch, fns, args.warmup, args.reps)
    rec = {"step": "center", "n": n, "values": {k: (None if v is None else float(v)) for k, v in values.items()},
           "equal": len({None if v is None else float(v) for v in values.values()}) == 1}
    rec.update({k: summary(t) for k, t in times.items()})
    rec["sharded_phases_ms"] = phases(torch, eng, fns["sharded_rank1_threadcomm"])
    return rec


def step_noise(args, torch, dev):
    from urh_amd.estimators import detect_noise_level_dev
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    n = 1 << args.log2n
    iq = capture(n, torch, dev)
    pipe, eng = DevicePipeline(0), GpuShardEngine(0)
    sp = ShardedPipeline(eng, ThreadComm(ThreadComm.Shared(1), 0))
    fns = {"sharded_rank1_threadcomm": lambda: sp.detect_noise_level(iq), "single": lambda: detect_noise_level_dev(pipe, iq)}
    values = {k: fn() for k, fn in fns.items()}
    times = alternating(torch, fns, args.warmup, args.reps)
    rec = {"step": "noise", "n": n, "values": values, "equal": len(set(values.values())) == 1}
    rec.update({k: summary(t) for k, t in times.items()})
    rec["sharded_phases_ms"] = phases(torch, eng, fns["sharded_rank1_threadcomm"])
    return rec


def step_rccl1(args, torch, dev):
    import torch.distributed as dist
    from urh_amd.estimators import detect_center_dev, detect_noise_level_dev
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import RcclComm, ShardedPipeline
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        comm = RcclComm.create()
        kind = type(comm).__name__
        n = 1 << args.log2n
        pipe, eng = DevicePipeline(0), GpuShardEngine(0)
        sp = ShardedPipeline(eng, comm)
        x = demodulated(n, torch, dev)
        rec = {"step": "rccl1", "n": n, "comm": kind, "fallback_reason": RcclComm.last_fallback_reason}
        want = detect_center_dev(pipe, x, _single=True)
        rec["center_equal"] = bool(sp.detect_center(x) == want)
        rec["center"] = summary(timed(torch, lambda: sp.detect_center(x), args.warmup, args.reps))
        del x
        iq = capture(n, torch, dev)
        rec["noise_equal"] = bool(sp.detect_noise_level(iq) == detect_noise_level_dev(pipe, iq))
        rec["noise"] = summary(timed(torch, lambda: sp.detect_noise_level(iq), args.warmup, args.reps))
        return rec
    finally:
        dist.destroy_process_group()


def step_threads8(args, torch, dev):
    import threading
    from urh_amd.estimators import detect_center_dev, detect_noise_level_dev
    from urh_amd.pipeline import DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm, shard_bounds
    n, world = 1 << args.log2n, 8
    pipe = DevicePipeline(0)
    engines = [GpuShardEngine(0) for _ in range(world)]
    bounds = shard_bounds(n, world)

    def ranks(call):
        shared = ThreadComm.Shared(world)
        out, err = [None] * world, []

        def work(r):
            try:
                out[r] = call(ShardedPipeline(engines[r], ThreadComm(shared, r)), r)
            except BaseException as e:          # noqa: BLE001
                err.append(e)
                shared.barrier.abort()
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if err:
            raise err[0]
        return out
    x = demodulated(n, torch, dev)
    want = detect_center_dev(pipe, x, _single=True)
    got = ranks(lambda sp, r: sp.detect_center(x[bounds[r][0]:bounds[r][1]]))
    rec = {"step": "threads8", "n": n, "center": None if want is None else float(want), "center_equal_on_every_rank": bool(all(g == want for g in got))}
    del x
    iq = capture(n, torch, dev)
    want = detect_noise_level_dev(pipe, iq)
    got = ranks(lambda sp, r: sp.detect_noise_level(iq[bounds[r][0]:bounds[r][1]], pos_base=bounds[r][0], n_total=n))
    rec.update({"noise": want, "noise_equal_on_every_rank": bool(all(g == want for g in got))})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "the probe needs a GPU"
        rec = globals()["step_" + args.step](args, torch, torch.device("cuda", 0))
        print("PROBE " + json.dumps(rec))
        return 0
    lines = []
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--log2n", str(args.log2n), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(json.dumps({"step": step, "error": f"no result within {limit} s"}))
            break
        found = [ln[6:] for ln in done.stdout.splitlines() if ln.startswith("PROBE ")]
        if done.returncode != 0 or not found:
            lines.append(json.dumps({"step": step, "error": f"exit status {done.returncode}", "stderr_tail": done.stderr[-1500:]}))
            if step == "rccl1" and done.returncode > 0:
                continue                        # a Python error where RCCL cannot be had: the remaining step does not depend on it
            break
        lines.append(found[-1])
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0 if all('"error"' not in ln for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
