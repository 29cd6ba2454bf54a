#!/usr/bin/env python3
"""Run the REAL reference (where it is importable through oracle/ref_python.py) on SESSIONS of small synthetic captures -- lists of captures
that share one parameter set and lie back to back in one buffer, what DevicePipeline.iq_to_bits_batch_records is given -- and record, per
capture, what ends up in the Message objects of ProtocolAnalyzer.get_protocol_from_signal: bits, pause, RSSI, timestamp, bit_sample_pos.
Each capture is opened alone, as the reference opens a file; for the automatic variants its own AutoInterpretation.detect_noise_level and
detect_center set the threshold and the center first (Signal.py:97-103; the configured center where detect_center gives None).
    -> tests/golden/batch_records/batch_records.npz   per session `<s>/iq` (the captures back to back) and `<s>/starts`; per session, variant
                                      and divisor `<s>|<variant>|<d>/i` = n_msg per capture (-1: the reference raised), msg_off, pauses, pos,
                                      pos_off behind their five lengths, `/b` = the bits, `/f` = [rssi, timestamp]: flat, message after
                                      message, capture after capture; per session and variant `<s>|<variant>/nc` = [noise, center] per
                                      capture (NaN: not detected / None)
    -> tests/golden/batch_records/batch_records.json  per session the Signal parameters, the variants, the divisors, the captures' names
Data only.  The sessions (tests/batch_record_cases.py loads them, tests/test_batch_records_*.py say what each is for):
    gain-<mod>-<dtype>   ASK and FSK for each of the five sample types, three captures whose noise floor and amplitude cycle over
                         noise_cases.STREAM_GAINS; variants plain, noise, center, both; ASK with divisors 1 and 8
    fsk4                 bits_per_symbol = 2
    geom-<dtype>         ASK float32 and int8: captures of 0, 1 and 2 samples, no message, 70 messages, a trailing message padded from a
                         short closing pause, a middle window that runs past the capture's end in front of a capture that starts with strong
                         samples and whose first message starts at its sample 0, pulse tables of 63, 64, 65 and 129 rows, a message boundary on
                         the 64-row seam, a middle bit inside row 64
    w<sps>-<dtype>       window lengths 1, 7, 8, 9, 127, 128, 129, 257 and 9000, two captures each, the second window clipped
    tiny                 300 captures of four to six messages, samples_per_symbol 2: more than 1024 messages

    python tests/golden/make_batch_records_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from make_msg_records_golden import MAXMAG, SAMPLE_RATE, TIMESTAMP, ask, base, fsk, to_dtype  # noqa: E402  (sets the reference up)

from urh.ainterpretation import AutoInterpretation  # noqa: E402
from urh.signalprocessing.IQArray import IQArray  # noqa: E402
from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer  # noqa: E402
from urh.signalprocessing.Signal import Signal  # noqa: E402

import noise_cases as nc  # noqa: E402

DTYPES = ["float32", "int8", "uint8", "int16", "uint16"]
VARIANTS = {"plain": (False, False), "noise": (True, False), "center": (False, True), "both": (True, True)}
TIMESTAMP_STEP = 10.25                 # capture k of a session was recorded at TIMESTAMP + k * TIMESTAMP_STEP


def noisy(mod, messages, sps, dtype, seed, sigma, amp, lead, tail):
    """make_msg_records_golden's ask / fsk on top of a noise floor: complex Gaussian noise of sigma per component everywhere, the symbols at
    amplitude amp (ASK: a zero at 0.4 amp); unsigned sample types keep both components positive"""
    rng = np.random.default_rng(seed)
    parts = [np.zeros(lead, np.complex128)]
    for symbols, pause in messages:
        s = np.repeat(np.array(symbols), sps)
        if mod == "ASK":
            ph = rng.uniform(0.2, np.pi / 2 - 0.2, len(s)) if dtype.startswith("u") else rng.uniform(0, 2 * np.pi, len(s))
            parts.append(np.where(s > 0, amp, 0.4 * amp) * np.exp(1j * ph))
        else:
            parts.append(amp * np.exp(2j * np.pi * np.cumsum(np.where(s > 0, 0.05, -0.05))))
        parts.append(np.zeros(pause, np.complex128))
    parts.append(np.zeros(tail, np.complex128))
    z = np.concatenate(parts)
    z = z + sigma * (rng.standard_normal(len(z)) + 1j * rng.standard_normal(len(z)))
    if dtype.startswith("u"):
        z = np.abs(z.real) + 1j * np.abs(z.imag)
    return to_dtype(z, dtype)


def patterned(bits_and_pauses, sps, dtype, lead):
    """an ASK capture without random numbers (long windows that still compress): the amplitude follows a sawtooth of period 97 around its level"""
    env = [np.zeros(lead)]
    for bits, pause in bits_and_pauses:
        env.append(np.repeat(np.where(np.array(bits) > 0, 0.6, 0.25), sps))
        env.append(np.zeros(pause))
    env = np.concatenate(env)
    i = np.arange(len(env))
    amp = env * (1.0 + 0.04 * ((i % 97) / 96.0 - 0.5))
    return to_dtype(amp * np.exp(1j * (0.3 + 0.9 * ((i % 13) / 12.0))), dtype)


def alternating(n, first=1):
    return [(first + i) % 2 for i in range(n)]


def sessions():
    rng = np.random.default_rng(4242)
    out = {}
    # ---- the gain sweep: what auto_noise / auto_center are for ----
    for mi, mod in enumerate(("ASK", "FSK")):
        for di, dt in enumerate(DTYPES):
            caps = []
            for c in range(3):
                sigma, amp = nc.STREAM_GAINS[(3 * di + c + mi) % len(nc.STREAM_GAINS)]
                msgs = [([1] + rng.integers(0, 2, int(rng.integers(9, 20))).tolist(), int(rng.integers(140, 220))) for _ in range(2)]
                caps.append((f"c{c}", noisy(mod, msgs, 10, dt, 500 + 50 * mi + 5 * di + c, sigma, amp, lead=120 + 13 * c, tail=40 + 7 * c)))
            p = base(mod, dt, 10, center=0.3 if mod == "ASK" else 0.0, divisors=[1, 8] if mod == "ASK" else [1])
            out[f"gain-{mod}-{dt}"] = (caps, p, list(VARIANTS))
    # ---- bits_per_symbol = 2 ----
    caps = []
    for c in range(3):
        sym = [(rng.integers(0, 4, 5 + 2 * c).tolist(), 300), (rng.integers(0, 4, 4 + c).tolist(), 0 if c == 1 else 280)]
        caps.append((f"c{c}", fsk(sym, 20, "int16", 60 + c, lead=9 + 10 * c, tones=(-0.06, -0.02, 0.02, 0.06), bps=2)))
    out["fsk4"] = (caps, base("FSK", "int16", 20, bits_per_symbol=2, center=0.0, center_spacing=float(np.float32(2 * np.pi * 0.04))), ["plain"])
    # ---- geometry: ASK, sps 5, a pause of more than 8 symbols closes a message ----
    for dt in ("float32", "int8"):
        seed = 700 if dt == "float32" else 800
        P, S = 60, 5
        clip = ask([([1, 0, 1, 1], P), ([1], 0)], S, dt, seed + 6)
        mid_bits = alternating(63) + [0, 0, 0] + alternating(63)                      # rows 1 .. 63 one bit each, row 64 three bits: bit 64 is its second
        caps = [
            ("n0", np.zeros((0, 2), dt)), ("n1", ask([([1], 0)], 1, dt, seed, lead=0)[:1]), ("n2", ask([([1], 0)], 2, dt, seed + 1, lead=0)[:2]),
            ("none", to_dtype(np.zeros(301, np.complex128), dt)),
            ("m70", ask([([1] + rng.integers(0, 2, 1 + m % 3).tolist(), 48 + m % 5) for m in range(70)], S, dt, seed + 2, lead=23)),
            ("pad", ask([([1], 100), ([1, 0, 1, 1, 1], 65), ([1, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1], 59), ([1, 0, 0, 1, 0, 1], 95), ([1, 0, 1], 0)], S, dt,
                        seed + 3)),
            ("trail", ask([([1, 0, 1], 150), ([1, 1], 27)], S, dt, seed + 4)),
            ("odd", ask([([1, 1, 0, 1], P), ([1, 0], P)], S, dt, seed + 5, lead=18)),
            ("clip", clip),                       # ends with one bit: its row begins a sample late (the tolerance) and its window runs a sample over
            ("at0", ask([([0, 1, 1, 0, 1, 0, 0, 1], P), ([1, 0, 1], P)], S, dt, seed + 7, lead=0)),      # (ASK slices sample 0 as a zero)
            ("r63", ask([(alternating(30), P), (alternating(30), P)], S, dt, seed + 8)),
            ("r64", ask([(alternating(31), P), (alternating(30), P)], S, dt, seed + 9)),
            ("r65", ask([(alternating(31), P), (alternating(31), P)], S, dt, seed + 10)),
            ("r129", ask([(alternating(31), P)] * 4, S, dt, seed + 11)),
            ("seam", ask([(alternating(62), P), (alternating(9), P)], S, dt, seed + 12)),      # the closing pause is row 63, the next message begins with row 64
            ("mid", ask([(mid_bits, P)], S, dt, seed + 13)),
        ]
        out[f"geom-{dt}"] = (caps, base("ASK", dt, S, divisors=[1, 8]), ["plain"])
    # ---- window lengths: two captures each; the second ends inside its last message's middle window ----
    for i, sps in enumerate([1, 7, 8, 9, 127, 128, 129, 257]):
        dt = "float32" if sps in (1, 7, 8, 9, 128) else "int8"
        a = ask([([1, 0, 1], 3 * sps), ([1, 1, 0], 3 * sps)], sps, dt, 900 + sps, lead=5 + i)
        b = ask([([1, 1], 3 * sps), ([1], 0)], sps, dt, 950 + sps, lead=3 + i)
        out[f"w{sps}-{dt}"] = ([("a", a), ("b", b[:len(b) - sps // 3])], base("ASK", dt, sps, pause_threshold=2), ["plain"])
    a = patterned([([1], 0)], 9100, "int8", lead=50)[:9150]
    b = patterned([([1], 0)], 9100, "int8", lead=31)[:31 + 8300]                # 0.92 symbols: the window is clipped to 8300 terms, more than one piece
    out["w9000-int8"] = ([("a", a), ("b", b)], base("ASK", "int8", 9000), ["plain"])
    # ---- 300 tiny captures: more messages than the records kernel's grid has workgroups ----
    caps = []
    for c in range(300):
        msgs = [([1] + rng.integers(0, 2, int(rng.integers(0, 3))).tolist(), 2 * int(rng.integers(3, 6))) for _ in range(4 + c % 3)]
        caps.append((f"t{c}", ask(msgs, 2, "int8", 2000 + c, lead=c % 5, jitter=0.0)))
    out["tiny"] = (caps, base("ASK", "int8", 2, pause_threshold=2, tolerance=0), ["plain"])
    return out


def interpret(iq, p, divisor, auto_noise, auto_center, timestamp):
    s = Signal("")
    s.iq_array = IQArray(np.array(iq))
    s.sample_rate, s.timestamp = SAMPLE_RATE, timestamp
    for k in ("modulation_type", "bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
              "costas_loop_bandwidth"):
        setattr(s, k, p[k])
    noise = center = float("nan")
    if auto_noise:
        noise = s.noise_threshold = AutoInterpretation.detect_noise_level(s.iq_array.magnitudes)
    if auto_center:
        c = AutoInterpretation.detect_center(np.array(s.qad), max_size=None)
        if c is not None:
            center = s.center = c
    s.message_length_divisor = divisor
    pa = ProtocolAnalyzer(s)
    pa.get_protocol_from_signal()
    return pa.messages, float(noise), float(center)


def main():
    arrays, meta = {}, {}
    for name, (caps, p, variants) in sessions().items():
        assert all(len(iq) <= 20000 for _, iq in caps), name
        arrays[f"{name}/iq"] = np.concatenate([iq for _, iq in caps])
        arrays[f"{name}/starts"] = np.concatenate([[0], np.cumsum([len(iq) for _, iq in caps])]).astype(np.int64)
        meta[name] = dict(p, sample_rate=SAMPLE_RATE, timestamp=TIMESTAMP, timestamp_step=TIMESTAMP_STEP, variants=variants, captures=[c for c, _ in caps])
        for v in variants:
            for d in p["divisors"]:
                per, noise, center = [], [], []
                for k, (cname, iq) in enumerate(caps):
                    with warnings.catch_warnings(), np.errstate(all="ignore"):
                        warnings.simplefilter("ignore")
                        try:
                            msgs, nz, ce = interpret(iq, p, d, *VARIANTS[v], TIMESTAMP + k * TIMESTAMP_STEP)
                        except (ValueError, OverflowError) as exc:
                            print(name, v, d, cname, "raises", type(exc).__name__, exc)
                            msgs, nz, ce = None, float("nan"), float("nan")
                    per.append(msgs)
                    noise.append(nz)
                    center.append(ce)
                flat = [m for msgs in per if msgs for m in msgs]
                bits = [list(m.plain_bits) for m in flat]
                pos = [[int(x) for x in m.bit_sample_pos] for m in flat]
                key = f"{name}|{v}|{d}/"
                n_msg = np.array([-1 if msgs is None else len(msgs) for msgs in per], dtype=np.int64)
                ints = [n_msg, np.concatenate([[0], np.cumsum([len(m) for m in bits])]), np.array([int(m.pause) for m in flat], dtype=np.int64),
                        np.array([x for m in pos for x in m], dtype=np.int64), np.concatenate([[0], np.cumsum([len(m) for m in pos])])]
                # three arrays per entry (a zip member costs more than these hold): the five integer tables behind their lengths, the bits,
                # and rssi / timestamp side by side
                arrays[key + "i"] = np.concatenate([[len(a) for a in ints]] + ints).astype(np.int64)
                arrays[key + "b"] = np.array([b for m in bits for b in m], dtype=np.uint8)
                arrays[key + "f"] = np.array([[float(m.rssi) for m in flat], [float(m.timestamp) for m in flat]], dtype=np.float64)
                arrays[f"{name}|{v}/nc"] = np.array([noise, center], dtype=np.float64)
                print(name, v, d, len(caps), "captures", len(flat), "messages", n_msg[:16].tolist())
    os.makedirs(os.path.join(HERE, "batch_records"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "batch_records", "batch_records.npz"), **arrays)
    json.dump(meta, open(os.path.join(HERE, "batch_records", "batch_records.json"), "w"), separators=(",", ":"))
    print(os.path.getsize(os.path.join(HERE, "batch_records", "batch_records.npz")), "bytes;",
          os.path.getsize(os.path.join(HERE, "msg_records", "msg_records.npz")), "is the limit")


if __name__ == "__main__":
    main()
