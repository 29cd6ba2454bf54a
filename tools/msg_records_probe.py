#!/usr/bin/env python3
"""Message records inside a pass: what they cost and what they replace, wall time with the results on the host.

Everything runs in ONE process after warm-up, the two sides of a comparison alternating inside every round; median and min - max over
ROUNDS rounds.  A side counts as faster only where the gap exceeds the other side's own spread.

  protocol  protocol.get_protocol_from_signal_dev (one pass with its records queued behind it, one hand-out) against the route it replaces:
            the pass, the hand-out, then protocol.messages_from_bits (torch gather of the RSSI windows, a copy back, numpy) -- ms per call.
            Captures: the golden two_participants_i8, and a bursty 2^27-sample complex64 2-FSK capture with 128 messages (bench.py's
            "bursty" variant: 10 465 symbols + a 2 076-sample gap per 2^20-sample segment, noise_threshold 0.2).
  stream    CaptureStream with msg_records against the same stream without, want_pos False and True, at 2^20 and 2^27 samples of the
            bursty generator -- ms per pass over PASSES pushes + flush.  A stream with records takes the ordinary route (tail behind the hot
            kernel, records behind the tail, pack + copy behind the records) where the stream without takes the staged route: the figure
            includes that route change.  "pos" without records is the alternative that ships bit_sample_pos and leaves the RSSI to the host.

    python tools/msg_records_probe.py [--out profiles/msg_records_probe.txt] [--sizes 1048576,134217728] [--tag run1]
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
CALLS = 5


def spread(values):
    return f"{statistics.median(values):9.4f}  ({min(values):.4f} - {max(values):.4f})"


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "msg_records_probe.txt"))
    ap.add_argument("--sizes", default="1048576,134217728")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from urh_amd import protocol
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.synth import spec_fsk_capture

    def emit(s):
        """print and APPEND to --out: the runs of one comparison end up in one file, each under its own heading (--tag)"""
        print(s, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(s + "\n")

    emit(f"msg_records_probe {args.tag}: {torch.cuda.get_device_name(0)}, ms until the results are on the host, median (min - max) of {ROUNDS} rounds, "
         "sides alternating in every round")
    dev = torch.device("cuda", 0)
    sizes = [int(x) for x in args.sizes.split(",")]
    p_burst = DemodParams("FSK", 1, 0.2, 0.0, 1.0, 5, 100, 0.1, 8, True)

    # ---- protocol: get_protocol_from_signal_dev against the route it replaces ----
    z = np.load(os.path.join(here, "tests", "golden", "two_participants_i8.npz"))
    p_gold = DemodParams(str(z["modulation_type"]), int(z["bits_per_symbol"]), float(z["noise_threshold"]), float(z["center"]), float(z["center_spacing"]),
                         int(z["tolerance"]), int(z["samples_per_symbol"]), float(z["costas_loop_bandwidth"]), int(z["pause_threshold"]), True)
    jobs = [("two_participants_i8", torch.from_numpy(z["iq"]).to(dev), p_gold)]
    big, _ = spec_fsk_capture(max(sizes) >> 20, dev, first_segment=0, sps=100, n_symbols=10465)
    jobs.append((f"bursty 2^{max(sizes).bit_length() - 1}", big, p_burst))
    pipe = DevicePipeline(0)
    for name, iq, p in jobs:
        def records():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                msgs = protocol.get_protocol_from_signal_dev(pipe, iq, p, message_length_divisor=1)
            return (time.perf_counter() - t0) * 1e3 / CALLS, msgs

        def replaced():
            t0 = time.perf_counter()
            for _ in range(CALLS):
                res = pipe.iq_to_bits_checked(iq, p, want_qad=True)
                data, pauses, bsp = res.messages()
                msgs = protocol.messages_from_bits(pipe, iq, p, data, pauses, bsp, 1)
            return (time.perf_counter() - t0) * 1e3 / CALLS, msgs

        for _ in range(2):
            records(); replaced()
        a, b = [], []
        for _ in range(ROUNDS):
            t, new = records(); a.append(t)
            t, old = replaced(); b.append(t)
        same = len(new) == len(old) and all(x.plain_bits == y.plain_bits and x.pause == y.pause and (x.rssi == y.rssi or (x.rssi != x.rssi and y.rssi != y.rssi))
                                            and x.timestamp == y.timestamp and x.bit_sample_pos == y.bit_sample_pos for x, y in zip(new, old))
        emit(f"protocol  {name:<22} {len(new):4d} messages   records {spread(a)}   replaced route {spread(b)}   replaced / records "
             f"{statistics.median(b) / statistics.median(a):.2f}   messages {'==' if same else '!='}")
    del jobs, big, pipe
    torch.cuda.empty_cache()

    # ---- stream: ms per pass with records against without ----
    for n in sizes:
        x, _ = spec_fsk_capture(n >> 20, dev, first_segment=0, sps=100, n_symbols=10465)
        pipes = {(rec, pos): DevicePipeline(0) for rec in (False, True) for pos in (False, True)}        # (a context of its own per stream)
        streams = {k: pipes[k].stream(n, replace(p_burst, write_bit_sample_pos=k[1]), want_qad=True, want_pos=k[1], msg_records=k[0]) for k in pipes}

        def run(st):
            t0 = time.perf_counter()
            n_msg = 0
            for _ in range(PASSES):
                r = st.push(x)
                if r is not None:
                    n_msg = r.check().n_msg
            for r in st.flush():
                n_msg = r.check().n_msg
            return (time.perf_counter() - t0) * 1e3 / PASSES, n_msg

        for _ in range(2):
            for st in streams.values():
                run(st)
        t = {k: [] for k in streams}
        for _ in range(ROUNDS):
            for k, st in streams.items():
                ms, n_msg = run(st)
                t[k].append(ms)
        for pos in (False, True):
            emit(f"stream    n = {n:>9}  {n_msg:4d} messages  want_pos {str(pos):<5}  without {spread(t[(False, pos)])}   with records {spread(t[(True, pos)])}   "
                 f"with / without {statistics.median(t[(True, pos)]) / statistics.median(t[(False, pos)]):.2f}")
        for st in streams.values():
            st.close()
        del x, streams, pipes
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
