#!/usr/bin/env python3
"""PSK captures one after the other: the one-shot loop against the capture stream, and what the device-driven Costas rounds cost.

For order-4 captures of 2^18, 2^20, 2^24 and 2^27 samples (seeded, carrier offset 0.04 cycles per sample, AWGN: the chunk chain never
breaks), warm-up first, then ROUNDS rounds in ONE process with the paths alternating inside every round; median and min - max:
  (a) per-capture wall time of K back-to-back captures as `pipe.iq_to_bits(d, p).host()` in a loop (host-driven rounds: the host waits
      inside every pass)
  (b) the same K captures through `pipe.stream(...)`: push, push, ..., flush
  (c) one empty predicated round: one-shot passes with costas_dev_rounds = 0 against = 8, the difference divided by 8 (costas.hip derives
      the number of rounds it queues from this figure: costas_auto_rounds)
  (d) 2^27 only: the one-shot pass with costas_dev_rounds = -1 (host-driven) against = 24

    python tools/psk_stream_probe.py [--out profiles/psk_stream_probe.txt] [--sizes 18,20,24,27]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 7


def psk_capture(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sym = torch.randint(0, 4, (n // 100 + 1,), generator=g, device="cuda")
    ph = (sym.double() * (torch.pi / 2) - 3 * torch.pi / 4).repeat_interleave(100)[:n] + 2 * torch.pi * 0.04 * torch.arange(n, device="cuda", dtype=torch.float64)
    iq = torch.stack([torch.cos(ph), torch.sin(ph)], 1).float()
    del ph
    return (iq + 0.1 * 0.5 ** 0.5 * torch.randn((n, 2), generator=g, device="cuda")).contiguous()


def spread(values):
    return f"{statistics.median(values):9.4f}  ({min(values):.4f} - {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "psk_stream_probe.txt"))
    ap.add_argument("--sizes", default="18,20,24,27")
    args = ap.parse_args()
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    p = DemodParams("PSK", 2, 0.2, 0.0, 1.5, 5, 100, 0.1, 8, True)
    lines = [f"psk_stream_probe: {torch.cuda.get_device_name(0)}, order 4, ms per capture, median (min - max) of {ROUNDS} rounds, paths alternating in every round"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    for e in (int(x) for x in args.sizes.split(",")):
        n = 1 << e
        k = 20 if e <= 20 else (10 if e <= 24 else 5)
        caps = [psk_capture(torch, n, 10 + j) for j in range(2)]              # (two captures taking turns: the inputs of passes in flight differ)
        torch.cuda.synchronize()
        plain = DevicePipeline(0)
        streamer = DevicePipeline(0)
        st = streamer.stream(n, p, want_qad=False, want_pos=True)
        fixed = {r: DevicePipeline(0, tuning={"costas_dev_rounds": r}) for r in (0, 8, 24)}

        def loop_a():
            t0 = time.perf_counter()
            for j in range(k):
                plain.iq_to_bits(caps[j & 1], p, want_qad=False).host()
            return (time.perf_counter() - t0) * 1e3 / k

        def loop_b():
            t0 = time.perf_counter()
            for j in range(k):
                r = st.push(caps[j & 1])
                if r is not None:
                    r.check()
            for r in st.flush():
                r.check()
            return (time.perf_counter() - t0) * 1e3 / k

        def one_shot(pipe, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                pipe.iq_to_bits(caps[0], p, want_qad=True)
                pipe.ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / reps

        reps = 10 if e <= 24 else 4
        for _ in range(2):                                                     # warm-up: every path, every shape
            loop_a(); loop_b()
            for pipe in list(fixed.values()) + [plain]:
                one_shot(pipe, 2)
        a, b, r0, r8, host, r24 = [], [], [], [], [], []
        for _ in range(ROUNDS):
            a.append(loop_a()); b.append(loop_b())
            r0.append(one_shot(fixed[0], reps)); r8.append(one_shot(fixed[8], reps))
            if e == 27:
                host.append(one_shot(plain, reps)); r24.append(one_shot(fixed[24], reps))
        chunks = (n - 1 + 4095) // 4096
        emit(f"n = 2^{e} ({chunks} chunks), K = {k}")
        emit(f"  (a) one-shot loop, .host()        {spread(a)}")
        emit(f"  (b) capture stream                {spread(b)}   costas stats {st.stats()['costas']}")
        emit(f"  (c) one-shot, 0 rounds queued     {spread(r0)}")
        emit(f"      one-shot, 8 rounds queued     {spread(r8)}")
        emit(f"      one empty round               {(statistics.median(r8) - statistics.median(r0)) / 8 * 1e3:9.2f} us")
        if e == 27:
            emit(f"  (d) one-shot, host-driven (-1)    {spread(host)}   stats {plain.ctx.costas_stats5()}")
            emit(f"      one-shot, 24 rounds queued    {spread(r24)}   stats {fixed[24].ctx.costas_stats5()}")
        st.close()
        del caps, plain, streamer, fixed, st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
