#!/usr/bin/env python3
"""DC correction: what urhgpu_dc_correct_dev costs, device time with the capture resident.

Every step is a process of its own under a time limit of its own; a step that faults, aborts or runs out of time ends the run (nothing more is
started on the GPU).  Per step: median and min - max of ROUNDS rounds after one warm-up call, stream-synchronised wall time.

  f32_dc       float32, uniform noise of amplitude 0.1 on a DC term of 1.0: the clean path (chunks derived from their speculation)
  f32_cliff    float32, (2^24, 1, -2^24, -1) repeated: exactly zero mean, every chunk re-evaluated serially -- the known cliff
  int16, int8  the integer route (exact sums, one subtract pass)
  copy         urhgpu_bench_copy_ceiling_dev over the same bytes as the float32 capture: what one read + one write of it cost
  numpy        the reference's expression on the host at 2^24 samples (times N / 2^24: it is linear)
  stream_N     ms per pass of a CaptureStream with dc_correction against the same stream without, N samples

    python tools/dc_probe.py [--n 134217728] [--out profiles/dc_probe.txt] [--steps f32_dc,f32_cliff,...]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
LIMITS = {"f32_dc": 120, "f32_cliff": 240, "int16": 120, "int8": 120, "copy": 120, "numpy": 120, "stream_1048576": 180, "stream_134217728": 300}


def spread(values):
    return f"{statistics.median(values):10.4f}  ({min(values):.4f} - {max(values):.4f})"


def step(name, n):
    import ctypes as C

    import numpy as np
    if name == "numpy":
        m = min(n, 1 << 24)
        x = (np.random.default_rng(0).uniform(-0.1, 0.1, (m, 2)) + 1.0).astype(np.float32)
        ms = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            _ = x - np.mean(x, axis=0)
            ms.append((time.perf_counter() - t0) * 1e3)
        return f"numpy x - mean(x, 0), float32, {m} samples on the host: {spread(ms)} ms  (x {n / m:g} for {n} samples: {statistics.median(ms) * n / m:.0f} ms)"
    import torch
    from urh_amd import _lib
    from urh_amd.filter import dc_correct_dev
    from urh_amd.pipeline import DemodParams, DevicePipeline
    pipe = DevicePipeline(0)
    dev = pipe.device

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def stats():
        out = (C.c_int64 * 4)()
        _lib.check(_lib.load().urhgpu_test_dc_stats(pipe.ctx.handle, out))
        return f"chunks per column {out[0]}, derived {out[1]} (as guessed {out[3]}), re-evaluated {out[2]}"

    if name in ("f32_dc", "f32_cliff"):
        if name == "f32_dc":
            x = torch.rand((n, 2), device=dev, dtype=torch.float32) * 0.2 + 0.9
        else:
            col = torch.tensor([2.0 ** 24, 1.0, -2.0 ** 24, -1.0], device=dev, dtype=torch.float32).repeat(n // 4 + 1)[:n]
            x = torch.stack([col, -col], dim=1).contiguous()
        out = torch.empty_like(x)
        ms = timed(lambda: dc_correct_dev(pipe, x, out=out))
        return f"{name}: float32, {n} samples, {x.numel() * 4 / 2 ** 30:.2f} GiB: {spread(ms)} ms  [{stats()}]"
    if name in ("int16", "int8"):
        tdt = getattr(torch, name)
        x = torch.randint(-100, 120, (n, 2), device=dev, dtype=tdt)
        out = torch.empty_like(x)
        ms = timed(lambda: dc_correct_dev(pipe, x, out=out))
        return f"{name}: {n} samples, {x.numel() * x.element_size() / 2 ** 30:.2f} GiB: {spread(ms)} ms"
    if name == "copy":
        x = torch.rand((n, 2), device=dev, dtype=torch.float32)
        out = torch.empty_like(x)
        pipe.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        ms = []
        for _ in range(ROUNDS + 1):
            one = C.c_float(0.0)
            _lib.check(_lib.load().urhgpu_bench_copy_ceiling_dev(pipe.ctx.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n, 0, 10, C.byref(one)))
            ms.append(float(one.value))
        return f"copy ceiling (shape 0), {n} float32 samples read + written: {spread(ms[1:])} ms per copy"
    if name.startswith("stream_"):
        from urh_amd.synth import fsk_capture
        m = int(name.split("_")[1])
        iq, _ = fsk_capture(max(1, m // (1 << 20)), dev, seed=1)
        iq = (iq[:m] * 0.5 + 0.2).contiguous()
        p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
        passes = 8
        res = {}
        for dc in (False, True, False, True):
            st = pipe.stream(len(iq), p, want_qad=False, want_pos=False, dc_correction=dc)

            def run():
                for _ in range(passes):
                    st.push(iq)
                st.flush()
            res.setdefault(dc, []).extend(v / passes for v in timed(run))
            st.close()
        return (f"{name}: FSK float32, {len(iq)} samples, ms per pass over {passes} pushes + flush: without {spread(res[False])}   "
                f"with dc_correction {spread(res[True])}")
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 27)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_probe.txt"))
    ap.add_argument("--steps", default="f32_dc,f32_cliff,int16,int8,copy,numpy,stream_1048576,stream_134217728")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its line")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + step(args.step, args.n), flush=True)
        return 0
    lines = [f"dc_probe: n = {args.n}, median (min - max) of {ROUNDS} rounds after one warm-up call, every step a process of its own"]
    print(lines[0], flush=True)
    status = 0
    for name in args.steps.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n)], capture_output=True, text=True,
                               timeout=LIMITS.get(name, 120))
            rc = r.returncode
            got = [l[7:] for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            line = got[0] if rc == 0 and got else f"{name}: FAILED rc={rc}: {(r.stderr or r.stdout).strip().splitlines()[-1:]}"
        except subprocess.TimeoutExpired:
            rc, line = 124, f"{name}: ran out of its {LIMITS.get(name, 120)} s"
        lines.append(line)
        print(line, flush=True)
        if rc != 0:
            status = 1
            lines.append("(stopped here: nothing more is started after a failed step)")
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
