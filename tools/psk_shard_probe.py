#!/usr/bin/env python3
"""Sharded PSK against one GPU on SURVEY 8(d) config 5 (urh_amd.synth.spec_psk_capture: 2^27 samples, 4-PSK, Costas bandwidth 0.1):

    single   DevicePipeline.iq_to_bits over the whole capture
    rank1    the sharded PSK pass with ONE rank (ShardedPipeline + GpuShardEngine + ThreadComm): its overhead over `single`
    threads8 8 ranks as threads on the one GPU (the ranks' kernels share it: a protocol check and a phase breakdown, not a scaling figure)

Times: median of --reps wall times of a whole pass, the GPU drained before and after.  Phases (one extra pass each, every phase
bracketed by a device synchronise): speculation + summary, exchange (all-gathers and the composition, resolves excluded), stitch + final,
pulse-table phases (last-value exchange, runs, rows, bits).  The exchange record (rounds, chunks by map / checkpoint / serial) comes from
ShardedPipeline.last_costas.

    python tools/psk_shard_probe.py [--segments 128] [--reps 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm, costas_halo_samples, shard_bounds, stitch
    from urh_amd.synth import spec_psk_capture
    dev = torch.device("cuda", 0)
    iq, _ = spec_psk_capture(args.segments, dev)
    n = iq.shape[0]
    p = DemodParams("PSK", 2, 0.2, 0.0, 1.5, 5, 100, 0.1, 8, True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    pipe = DevicePipeline(0)
    single_fn = lambda: pipe.iq_to_bits(iq, p, want_qad=True)      # noqa: E731
    res, _ = timed(single_fn)
    want = (res.ppseq().copy(),) + tuple(x.copy() for x in res.flat())
    want_qad = res.qad.cpu().numpy().copy()
    single_ms = statistics.median(timed(single_fn)[1] for _ in range(args.reps))
    single_stats = pipe.ctx.costas_stats()

    engines = [GpuShardEngine(0) for _ in range(8)]
    phase_ms = {}

    def instrument(eng, rank):
        """wrap the engine's phases with device-synchronised timers (phase pass only)"""
        def wrap(name, key):
            f = getattr(eng, name)

            def g(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f(*a, **k)
                torch.cuda.synchronize()
                phase_ms.setdefault(rank, {}).setdefault(key, 0.0)
                phase_ms[rank][key] += (time.perf_counter() - t0) * 1e3
                return r
            setattr(eng, name, g)
        for name, key in (("costas_spec", "speculate_summary"), ("costas_resolve", "stitch_final"), ("runs", "pulse_runs"),
                          ("rows", "pulse_rows"), ("bits_prepare", "pulse_bits_prepare"), ("bits_finish", "pulse_bits_finish")):
            wrap(name, key)

    def sharded(world, phases=False):
        bounds = shard_bounds(n, world)
        shared = ThreadComm.Shared(world)
        out, recs, err = [None] * world, [None] * world, []
        H = costas_halo_samples(p.costas_loop_bandwidth)
        if phases:
            for r in range(world):
                instrument(engines[r], r)

        def work(r):
            try:
                a, b = bounds[r]
                sp = ShardedPipeline(engines[r], ThreadComm(shared, r))
                t0 = time.perf_counter()
                out[r] = sp.iq_to_bits(iq[a:b], p, want_qad=True, pos_base=a, n_total=n, left_raw=iq[max(0, a - H):a] if r else None)
                torch.cuda.synchronize()
                recs[r] = dict(sp.last_costas, pass_ms=(time.perf_counter() - t0) * 1e3)
            except BaseException as e:          # noqa: BLE001
                err.append(e)
                shared.barrier.abort()
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        if err:
            raise err[0]
        return out, recs, (time.perf_counter() - t0) * 1e3

    rec = {"workload": f"configs[4] (SURVEY 8(d) config 5): {n} samples 4-PSK, Costas bandwidth 0.1, center 0, spacing 1.5, bits",
           "single_gpu": {"ms_median": round(single_ms, 3), "costas_chunks": single_stats}}
    for world, tag in ((1, "rank1"), (8, "threads8")):
        out, recs, _ = sharded(world)                   # warm-up + exactness
        got = stitch(out)
        exact = all(np.array_equal(a, b) for a, b in zip(got, want))
        got_qad = np.concatenate([r.qad.cpu().numpy() for r in out])
        exact = exact and np.array_equal(got_qad.view(np.uint32), want_qad.view(np.uint32))
        times = [sharded(world)[2] for _ in range(args.reps)]
        phase_ms.clear()
        _, precs, _ = sharded(world, phases=True)
        engines = [GpuShardEngine(0) for _ in range(8)]   # fresh, un-instrumented engines for the next configuration
        ms = statistics.median(times)
        rec[tag] = {"ranks": world, "ms_median": round(ms, 3), "ms_all": [round(t, 3) for t in times], "bit_exact": bool(exact),
                    "costas": recs, "phases_ms_per_rank": {str(r): {k: round(v, 3) for k, v in d.items()} for r, d in sorted(phase_ms.items())},
                    "phase_pass_ms_per_rank": [round(r["pass_ms"], 3) for r in precs]}
        for r, d in phase_ms.items():
            rest = precs[r]["pass_ms"] - sum(d.values())
            rec[tag]["phases_ms_per_rank"][str(r)]["exchange_and_host"] = round(rest, 3)
        if tag == "rank1":
            rec[tag]["ratio_to_single"] = round(ms / single_ms, 4)
    line = json.dumps(rec, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
