#!/usr/bin/env python3
"""Run the REAL reference's ProtocolAnalyzer.get_protocol_from_signal (where it is importable through oracle/ref_python.py) on small
synthetic captures built for the message records a pass ends with (include/urhgpu.h: urhgpu_msg_record) and record inputs and what
ends up in the Message objects: bits, pause, RSSI, timestamp, bit_sample_pos.
    -> tests/golden/msg_records/msg_records.npz   per case the capture `<case>/iq`, per case and divisor `<case>|<divisor>/{bits, msg_off, pauses,
                                      pos, pos_off, rssi, timestamp}` (flat, message after message)
    -> tests/golden/msg_records/msg_records.json  per case the Signal parameters and the divisors
Data only.  The cases (tests/test_msg_records_*.py say what each is for):
    w<sps>-<dtype>    window lengths 1, 7, 8, 9, 15, 16, 127, 128, 129, 136, 257, 300 and 9000, the five sample types in turn
    pad               ASK, divisors 1, 2 and 8: a 1-bit message padded to 8, a pause one sample too short, a pause of exactly
                      sps * missing, an odd and an even length, a trailing message without a pause
    trail, trail1     a trailing message whose capture ends in a short pause: it is padded from that pause
    clip, at0         a middle window that runs past the capture's end; a message that starts at sample 0
    fsk4              bits_per_symbol = 2
    none, one, m70, m1500   message counts
    u16nan, i8full    a uint16 sample whose magnitude sum wraps negative; int8 at full scale
    sa0..5, sf0..3    two families that share their parameters (ASK float32 with divisor 8, FSK int8): the pushes of a capture stream

    python tests/golden/make_msg_records_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_python  # noqa: E402

ref_python.setup()
from urh.signalprocessing.IQArray import IQArray  # noqa: E402
from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer  # noqa: E402
from urh.signalprocessing.Signal import Signal  # noqa: E402

SAMPLE_RATE, TIMESTAMP = 2e6, 1000.5
FULL = {"int8": 127.0, "uint8": 255.0, "int16": 32767.0, "uint16": 65535.0, "float32": 1.0}          # largest component
MAXMAG = {"int8": np.sqrt(127.0 ** 2 + 128.0 ** 2), "uint8": 255.0, "int16": np.sqrt(32768.0 ** 2 + 32767.0 ** 2), "uint16": 65535.0,
          "float32": np.sqrt(2.0)}                                                                      # afp_demod's max_magnitude


def to_dtype(c, dtype):
    """complex samples of magnitude <= 1 (relative to max_magnitude) as (N, 2) of dtype"""
    scale = MAXMAG[dtype]
    iq = np.stack([c.real, c.imag], axis=1) * scale
    if dtype == "float32":
        return iq.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.rint(iq), info.min, info.max).astype(dtype)


def ask(messages, sps, dtype, seed, lead=37, jitter=0.02):
    """messages: [(bits, samples of silence after them)]; 1 -> magnitude 0.6, 0 -> 0.25 (relative), silence exactly 0; unsigned sample
    types keep both components positive"""
    rng = np.random.default_rng(seed)
    env = [np.zeros(lead)]
    for bits, pause in messages:
        env.append(np.repeat(np.where(np.array(bits) > 0, 0.6, 0.25), sps))
        env.append(np.zeros(pause))
    env = np.concatenate(env)
    amp = env * (1.0 + jitter * rng.standard_normal(len(env)))
    phase = rng.uniform(0.1, np.pi / 2 - 0.1, len(env)) if dtype.startswith("u") else rng.uniform(0, 2 * np.pi, len(env))
    return to_dtype(amp * np.exp(1j * phase), dtype)


def fsk(messages, sps, dtype, seed, lead=37, tones=(-0.05, 0.05), bps=1):
    """messages: [(symbols, samples of silence after them)]; symbol k -> tones[k] cycles per sample, magnitude 0.5 (relative)"""
    rng = np.random.default_rng(seed)
    out = [np.zeros(lead, np.complex128)]
    for symbols, pause in messages:
        f = np.repeat(np.array(tones)[np.array(symbols)], sps)
        amp = 0.5 * (1.0 + 0.02 * rng.standard_normal(len(f)))
        out.append(amp * np.exp(2j * np.pi * np.cumsum(f)))
        out.append(np.zeros(pause, np.complex128))
    return to_dtype(np.concatenate(out), dtype)


def base(mod, dtype, sps, **kw):
    p = dict(modulation_type=mod, bits_per_symbol=1, noise_threshold=0.05 * MAXMAG[dtype], center=0.42 if mod == "ASK" else 0.0, center_spacing=1.0,
             tolerance=min(5, max(0, sps // 4)), samples_per_symbol=sps, pause_threshold=8, costas_loop_bandwidth=0.1, divisors=[1], dtype=dtype)
    p.update(kw)
    return p


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    dtypes = ["float32", "int8", "uint8", "int16", "uint16"]
    for i, sps in enumerate([1, 7, 8, 9, 15, 16, 127, 128, 129, 136, 257, 300]):
        dt = dtypes[i % 5]
        n_msg = 3 if sps <= 136 else 2
        msgs = [([1] + rng.integers(0, 2, 6 + m).tolist(), (12 + m) * sps) for m in range(n_msg)]
        out[f"w{sps}-{dt}"] = (ask(msgs, sps, dt, 100 + sps), base("ASK", dt, sps))
    # one window past 8192 terms: a trailing 1-bit message of 9100 samples
    out["w9000-float32"] = (ask([([1], 0)], 9100, "float32", 9000, lead=50)[:9150], base("ASK", "float32", 9000))
    # ASK padding, sps 10, pause_threshold 2 (a pause of 25 samples and more closes a message)
    pad = [([1], 200),                       # 1 bit, padded to 8 (and to 2): the middle index lies in the padded part
           ([1, 0, 1, 1, 1], 30),            # L = 5, divisor 8: missing 3, pause exactly 3 * sps -> padded, pause 0
           ([1, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 1], 29),   # L = 13, missing 3, pause one sample short -> not padded by 8 (by 2: yes)
           ([1, 0, 0, 1, 0, 1], 90),         # even L = 6: missing 2
           ([1, 1, 1, 0, 1, 0, 1, 1], 60),   # L = 8: nothing missing for 8 and 2
           ([1, 0, 1], 0)]                   # trailing, no pause behind it: nothing to borrow
    out["pad"] = (ask(pad, 10, "float32", 7), base("ASK", "float32", 10, pause_threshold=2, divisors=[1, 2, 8]))
    # a TRAILING message is padded too when the capture ends in a pause too short to close it: that pause's symbols count as zero bits AND
    # its samples are the message's pause.  2 bits + 5.4 symbols of silence: 7 bits, one more borrowed; 3 bits + 2.7 symbols: 6 bits, two more
    out["trail"] = (ask([([1, 0, 1], 300), ([1, 1], 54)], 10, "float32", 21), base("ASK", "float32", 10, divisors=[1, 2, 8]))
    out["trail1"] = (ask([([1, 1], 300), ([1, 0, 1], 27)], 10, "uint8", 22), base("ASK", "uint8", 10, divisors=[1, 8]))
    out["pad-i16"] = (ask(pad, 10, "int16", 8), base("ASK", "int16", 10, pause_threshold=2, divisors=[1, 2, 8]))
    # the middle window runs past the end: a trailing message of one bit, 0.7 symbols long
    clip = ask([([1, 0, 1, 1], 400), ([1], 0)], 40, "float32", 11)
    out["clip"] = (clip[:len(clip) - 12], base("ASK", "float32", 40))
    # (afp_demod writes NOISE into sample 0, which ASK slices as a zero: a message starts at sample 0 when its first bit is a zero)
    out["at0"] = (ask([([0, 1, 1, 0, 1, 0, 0, 1], 300), ([1, 0, 1], 250)], 20, "int8", 12, lead=0), base("ASK", "int8", 20, divisors=[1, 8]))
    sym = [(rng.integers(0, 4, 9).tolist(), 400), (rng.integers(0, 4, 6).tolist(), 350), (rng.integers(0, 4, 5).tolist(), 0)]
    out["fsk4"] = (fsk(sym, 30, "float32", 13, tones=(-0.06, -0.02, 0.02, 0.06), bps=2),
                   base("FSK", "float32", 30, bits_per_symbol=2, center=0.0, center_spacing=float(np.float32(2 * np.pi * 0.04))))
    out["fsk-i16"] = (fsk([(rng.integers(0, 2, 12).tolist(), 700), (rng.integers(0, 2, 7).tolist(), 0)], 50, "int16", 14), base("FSK", "int16", 50))
    out["none"] = (to_dtype(np.zeros(600, np.complex128), "float32"), base("ASK", "float32", 20))
    out["one"] = (ask([([1, 0, 1, 1, 0], 0)], 20, "uint8", 15), base("ASK", "uint8", 20, divisors=[1, 8]))
    out["m70"] = (ask([([1] + rng.integers(0, 2, 1 + m % 5).tolist(), 10 * 8 + m % 7) for m in range(70)], 8, "float32", 16),
                  base("ASK", "float32", 8, divisors=[1, 8]))
    out["m1500"] = (ask([([1] + rng.integers(0, 2, 2 + m % 3).tolist(), 4 + m % 3) for m in range(1500)], 1, "int8", 17, jitter=0.0),
                    base("ASK", "int8", 1, pause_threshold=2, divisors=[1, 2]))
    # a uint16 sample whose magnitude sum wraps negative inside the middle window of the first message
    u16 = ask([([1, 0, 1, 1, 0, 1, 1], 500), ([1, 1, 0, 1], 450)], 30, "uint16", 18)
    u16[37 + 3 * 30 + 11] = (40000, 40000)
    out["u16nan"] = (u16, base("ASK", "uint16", 30))
    i8 = ask([([1, 1, 0, 1, 1, 0, 1], 300), ([1, 0, 1, 1, 1], 280)], 20, "int8", 19)
    on = np.abs(i8.astype(np.int32)).sum(axis=1) > 60
    i8[on] = np.where(np.arange(len(i8))[on, None] % 2 == 0, np.int8(-128), np.int8(127))            # full scale, both ends of the range
    out["i8full"] = (i8, base("ASK", "int8", 20, center=0.6))
    # two families of captures that share their parameters: what a capture stream is pushed, interleaved
    for i in range(6):
        msgs = [([1] + rng.integers(0, 2, rng.integers(0, 14)).tolist(), int(rng.integers(25, 140))) for _ in range(3 + 2 * i)]
        out[f"sa{i}"] = (ask(msgs, 10, "float32", 30 + i, lead=11 + 7 * i), base("ASK", "float32", 10, pause_threshold=2, divisors=[1, 8]))
    for i in range(4):
        msgs = [(rng.integers(0, 2, rng.integers(3, 20)).tolist(), int(rng.integers(260, 500))) for _ in range(2 + 3 * i)]
        out[f"sf{i}"] = (fsk(msgs, 25, "int8", 40 + i, lead=5 + 9 * i), base("FSK", "int8", 25))
    return out


def run(iq, p, divisor):
    s = Signal("")
    s.iq_array = IQArray(iq)
    s.sample_rate, s.timestamp = SAMPLE_RATE, TIMESTAMP
    for k in ("modulation_type", "bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
              "costas_loop_bandwidth"):
        setattr(s, k, p[k])
    s.message_length_divisor = divisor
    pa = ProtocolAnalyzer(s)
    with np.errstate(all="ignore"):
        pa.get_protocol_from_signal()
    return pa.messages


def main():
    arrays, meta = {}, {}
    for name, (iq, p) in cases().items():
        assert len(iq) <= 20000, (name, len(iq))
        arrays[f"{name}/iq"] = iq
        meta[name] = dict(p, sample_rate=SAMPLE_RATE, timestamp=TIMESTAMP, n=len(iq))
        for d in p["divisors"]:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                msgs = run(iq, p, d)
            bits = [list(m.plain_bits) for m in msgs]
            pos = [[int(v) for v in m.bit_sample_pos] for m in msgs]
            key = f"{name}|{d}/"
            arrays[key + "bits"] = np.array([b for m in bits for b in m], dtype=np.uint8)
            arrays[key + "msg_off"] = np.concatenate([[0], np.cumsum([len(m) for m in bits])]).astype(np.int64)
            arrays[key + "pauses"] = np.array([int(m.pause) for m in msgs], dtype=np.int64)
            arrays[key + "pos"] = np.array([v for m in pos for v in m], dtype=np.int64)
            arrays[key + "pos_off"] = np.concatenate([[0], np.cumsum([len(m) for m in pos])]).astype(np.int64)
            arrays[key + "rssi"] = np.array([float(m.rssi) for m in msgs], dtype=np.float64)
            arrays[key + "timestamp"] = np.array([float(m.timestamp) for m in msgs], dtype=np.float64)
            print(name, d, len(iq), len(msgs), [len(b) for b in bits[:8]], [int(m.pause) for m in msgs[:8]], [round(float(m.rssi), 4) for m in msgs[:4]])
    os.makedirs(os.path.join(HERE, "msg_records"), exist_ok=True)      # (a directory of its own: the .npz files directly under tests/golden/ are the golden captures)
    np.savez_compressed(os.path.join(HERE, "msg_records", "msg_records.npz"), **arrays)
    json.dump(meta, open(os.path.join(HERE, "msg_records", "msg_records.json"), "w"), separators=(",", ":"))


if __name__ == "__main__":
    main()
