#!/usr/bin/env python3
"""What a live chunk costs: sustained samples per second through LiveSniffer.feed, against what a user of the public API could
write without it (torch expressions for the noise gate on the device, a torch copy into a buffer, DevicePipeline.iq_to_bits on
flush).

    python tools/sniffer_probe.py [--dtypes float32,int8] [--chunks 20000,200000,2000000] [--out FILE]

The stream is host memory, as in live reception: numpy chunks of a 2-FSK transmission (sps 100), six chunks of signal followed by
two of noise, so that every cycle of eight chunks ends in one flush over six chunks' rows.  Both paths see the same chunks, make
the same decisions (checked: flushes and message counts must agree) and end every chunk with one synchronisation.

Every (dtype, chunk size) is measured in a child process of its own under a time limit; in it the two paths alternate, round by
round, after one warm-up cycle each.  The figure is rows fed / wall time of a round (the median over the rounds, with the
spread).  After a child that failed or ran out of time nothing more is started.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPS = 100
SIGNAL_CHUNKS, NOISE_CHUNKS = 6, 2


def make_chunks(n, dtype, seed=3):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n // SPS + 1)
    f = np.repeat(np.where(bits == 1, 0.05, -0.05), SPS)[:n]
    ph = np.cumsum(f)
    sig = 0.7 * np.stack([np.cos(ph), np.sin(ph)], axis=1) + 0.01 * rng.standard_normal((n, 2))
    noise = 0.01 * rng.standard_normal((n, 2))
    if np.dtype(dtype) == np.float32:
        return sig.astype(np.float32), noise.astype(np.float32), 0.1
    info = np.iinfo(dtype)
    scale = (info.max - info.min) / 2
    conv = lambda x: np.clip(np.round(x * scale), info.min, info.max).astype(dtype)     # noqa: E731
    return conv(sig), conv(noise), 0.1 * scale


class TorchSniffer:
    """the reference's per-chunk procedure (ProtocolSniffer.py:204-281, no adaptive noise) with what the package offered before
    urh_amd.sniffer: torch for the gate and the append, DevicePipeline.iq_to_bits for the flush"""

    def __init__(self, pipe, params, dtype, buffer_samples):
        import torch
        self.torch, self.pipe, self.p = torch, pipe, params
        self.tdtype = getattr(torch, np.dtype(dtype).name)
        self.acc = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
        self.buffer = torch.empty((buffer_samples, 2), dtype=self.tdtype, device=pipe.device)
        self.index, self.pause_length, self.n_messages, self.flushes = 0, 0, 0, 0

    def feed(self, chunk):
        torch = self.torch
        n = len(chunk)
        d = torch.from_numpy(chunk).to(self.pipe.device)
        ps = d.to(self.acc) ** 2.0
        rms = math.sqrt(float(ps.mean()))                    # one synchronisation (no adaptive noise: the maximum is not needed)
        if rms > self.p.noise_threshold:
            self._append(d, n)
            self.pause_length = 0
            if self.index < len(self.buffer) - 2:
                return
        else:
            self.pause_length += n
            if self.pause_length < 10 * self.p.samples_per_symbol:
                self._append(d, n)
                if self.index < len(self.buffer) - 2:
                    return
        if self.index == 0:
            return
        res = self.pipe.iq_to_bits_checked(self.buffer[:self.index], self.p, want_qad=False)
        self.index = 0
        self.n_messages += len(res.messages()[0])
        self.flushes += 1

    def _append(self, d, n):
        if n + self.index > len(self.buffer):
            n = len(self.buffer) - self.index - 1
        self.buffer[self.index:self.index + n].copy_(d[:n])
        self.index += n


def child(dtype, n, rounds, cycles):
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.sniffer import LiveSniffer
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dtype = np.dtype(dtype)
    sig, noise, thr = make_chunks(n, dtype)
    cycle = [sig] * SIGNAL_CHUNKS + [noise] * NOISE_CHUNKS
    pipe = DevicePipeline(0)
    p = DemodParams("FSK", 1, thr, 0.0, 1.0, 5, SPS, 0.1, 8, True)
    rows_buf = max(12_500_000, (SIGNAL_CHUNKS + 1) * n)
    new = LiveSniffer(pipe, p, dtype=dtype, buffer_samples=rows_buf, trace=False)
    old = TorchSniffer(pipe, p, dtype, rows_buf)

    def run(sn, k):
        t0 = time.perf_counter()
        for _ in range(k):
            for c in cycle:
                sn.feed(c)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for sn in (new, old):
        run(sn, 1)                                           # warm-up: code objects, buffers, the pinned staging area
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(run(new, cycles))
        t_old.append(run(old, cycles))
    n_flush_new = sum(1 for _ in new.centers)
    assert n_flush_new == old.flushes and len(new.messages) == old.n_messages, (n_flush_new, old.flushes, len(new.messages), old.n_messages)
    rows = cycles * len(cycle) * n
    rate = lambda ts: [rows / t for t in ts]                 # noqa: E731
    out = {"dtype": dtype.name, "chunk_rows": n, "rounds": rounds, "rows_per_round": rows, "flushes": old.flushes, "messages": old.n_messages,
           "device": torch.cuda.get_device_name(0)}
    for name, ts in (("live_sniffer", t_new), ("torch_public_api", t_old)):
        r = sorted(rate(ts))
        out[name] = {"rows_per_s_median": r[len(r) // 2], "rows_per_s_min": r[0], "rows_per_s_max": r[-1],
                     "us_per_chunk_median": 1e6 * sorted(ts)[len(ts) // 2] / (cycles * len(cycle))}
    out["ratio_new_over_torch"] = out["live_sniffer"]["rows_per_s_median"] / out["torch_public_api"]["rows_per_s_median"]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="float32,int8")
    ap.add_argument("--chunks", default="20000,200000,2000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per (dtype, chunk size) child")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=4, metavar=("DTYPE", "ROWS", "ROUNDS", "CYCLES"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]))
        return 0
    results = []
    for dt in a.dtypes.split(","):
        for n in (int(v) for v in a.chunks.split(",")):
            cycles = max(2, min(60, 8_000_000 // (n * (SIGNAL_CHUNKS + NOISE_CHUNKS))))      # about 8 M rows per round, at least two cycles
            cmd = [sys.executable, os.path.abspath(__file__), "--child", dt, str(n), str(a.rounds), str(cycles)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"{dt} / {n} rows: no result within {a.timeout} s -- stopping", flush=True)
                return 124
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"{dt} / {n} rows: child failed with status {r.returncode} -- stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
                return r.returncode or 1
            res = json.loads(line[0][7:])
            results.append(res)
            print(f"{dt:8s} chunk {n:8d} rows: LiveSniffer {res['live_sniffer']['rows_per_s_median'] / 1e6:9.1f} M rows/s "
                  f"({res['live_sniffer']['us_per_chunk_median']:9.1f} us/chunk)   torch + public API "
                  f"{res['torch_public_api']['rows_per_s_median'] / 1e6:9.1f} M rows/s ({res['torch_public_api']['us_per_chunk_median']:9.1f} us/chunk)"
                  f"   ratio {res['ratio_new_over_torch']:.2f}", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
