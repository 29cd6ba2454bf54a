#!/usr/bin/env python3
"""Generate tests/golden/sniffer/*.npz by driving the REAL reference's live mode,
ProtocolSniffer.__demodulate_data (src/urh/signalprocessing/ProtocolSniffer.py:204-281), chunk by chunk over seeded synthetic
captures.  The reference tree does not exist where the GPU tests run, so the vectors are committed; re-run this script only
when cases are added.

    python tests/golden/make_sniffer_golden.py

ProtocolSniffer.__init__ builds a VirtualDevice (SDR backends, Qt signals) that the PyQt6 stub cannot serve, so the object is
made with __new__, given the two base-class initialisations __init__ performs and a stand-in receive device that has only
`sample_rate` and `data_type`; everything __demodulate_data touches is then the reference's own code.  time.time is patched to
a constant so that the message timestamps are reproducible.

Each case stores the capture, the chunk lengths, the parameters and
  after every chunk   above-noise (-1: empty chunk, nothing decided), the noise threshold (as float64) AND the name of its scalar
                      type, pause_length, the buffer index, the message count
  per flush           the center the messages were sliced with
  per message         bits, pause, the first bit's sample position, the timestamp (absolute, at the patched clock)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "sniffer")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_python  # noqa: E402

ref_python.setup()
sys.modules.setdefault("PyQt6.uic", types.ModuleType("PyQt6.uic"))
from PyQt6.QtCore import QObject  # noqa: E402
import urh.signalprocessing.ProtocolSniffer as PS  # noqa: E402
from urh.signalprocessing.IQArray import IQArray  # noqa: E402
from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer  # noqa: E402
from urh.signalprocessing.Signal import Signal  # noqa: E402

CLOCK = 1700000000.25
SAMPLE_RATE = 1e6


class _Log:
    """counts the reference's "Buffer of protocol sniffer is full" warnings: one per trimmed append"""
    def __init__(self):
        self.trims = 0

    def warning(self, *a, **k):
        self.trims += 1

    def __getattr__(self, name):
        return lambda *a, **k: None


def make_sniffer(mod, sps, bps, center, spacing, noise, tolerance, dtype, adaptive, autocenter, buffer_mb):
    signal = Signal("", "LiveSignal")                       # as ProtocolSniffer.__init__ (:45-55)
    signal.samples_per_symbol = sps
    signal.center = center
    signal.center_spacing = spacing
    signal.noise_threshold = noise
    signal.tolerance = tolerance
    signal.silent_set_modulation_type(mod)
    signal.bits_per_symbol = bps
    sn = PS.ProtocolSniffer.__new__(PS.ProtocolSniffer)
    ProtocolAnalyzer.__init__(sn, signal)
    QObject.__init__(sn, None)
    sn.rcv_device = types.SimpleNamespace(sample_rate=SAMPLE_RATE, data_type=dtype)
    signal.iq_array = IQArray(None, dtype, 0)
    sn.BUFFER_SIZE_MB = buffer_mb
    sn._ProtocolSniffer__init_buffer()
    sn.adaptive_noise = adaptive
    sn.automatic_center = autocenter
    sn.pause_length = 0
    return sn


# ---- seeded captures: bursts of `nbits` random bits separated by noise ---------------------------------------------------------
def capture(mod, bps, sps, n_msgs, nbits, gap, seed, dtype=np.float32, amp=0.7, sigma=0.01, lead=None):
    rng = np.random.default_rng(seed)
    parts = [np.zeros(gap if lead is None else lead, np.complex128)]
    for _ in range(n_msgs):
        sym = rng.integers(0, 1 << bps, nbits // bps)
        sym[0] = (1 << bps) - 1                              # a message starts with energy (ASK) / a defined symbol
        lvl = np.repeat(sym, sps).astype(np.float64)
        if mod == "FSK":
            step = 0.1                                       # rad / sample between neighbouring symbols, centred on 0
            f = (lvl - ((1 << bps) - 1) / 2) * step
            burst = amp * np.exp(1j * np.cumsum(f))
        elif mod == "ASK":
            burst = amp * lvl * np.exp(1j * 0.05 * np.arange(len(lvl)))
        else:                                                # PSK: 0 / pi on a carrier of 0.01 cycles per sample
            burst = amp * np.exp(1j * (2 * np.pi * 0.01 * np.arange(len(lvl)) + np.pi * lvl))
        parts += [burst, np.zeros(gap + int(rng.integers(0, 3 * sps)), np.complex128)]
    x = np.concatenate(parts)
    x = x + sigma * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    iq = np.stack([x.real, x.imag], axis=1)
    if np.dtype(dtype) == np.float32:
        return np.ascontiguousarray(iq.astype(np.float32))
    info = np.iinfo(dtype)
    scale = (info.max - info.min) / 2
    off = (info.max + info.min + 1) / 2
    return np.ascontiguousarray(np.clip(np.round(iq * scale + off), info.min, info.max).astype(dtype))


def chunk_lengths(n, lo, hi, seed, head=()):
    rng = np.random.default_rng(seed)
    out = list(head)
    left = n - sum(out)
    while left > 0:
        c = int(min(rng.integers(lo, hi + 1), left))
        out.append(c)
        left -= c
    return np.asarray(out, np.int64)


def run_case(name, iq, lens, mod, sps, bps=1, center=0.0, spacing=1.0, noise=0.1, tolerance=5, adaptive=False, autocenter=False,
             buffer_mb=100, min_msgs=3, want_trim=False, qad0=None):
    dtype = iq.dtype
    if mod == "PSK" and qad0 is None:
        # costa_demod never writes result[0] of its np.empty array (signal_functions.pyx:265, :289), and the first pulse, the first bit position
        # and even the message lengths depend on that sample: what the reference answers for a PSK flush is partly uninitialised memory.
        # The fixture pins the run in which that one sample holds the value this project's library documents for it (include/urhgpu.h,
        # urhgpu_afp_demod: the noise marker -4.0); every other sample is the reference's own
        qad0 = -4.0
    sn = make_sniffer(mod, sps, bps, center, spacing, noise, tolerance, dtype, adaptive, autocenter, buffer_mb)
    log = _Log()
    PS.logger = log
    PS.time = types.SimpleNamespace(time=lambda: CLOCK)
    flushes = []
    inner = sn._ppseq_to_bits

    def counted(*a, **k):
        flushes.append(float(sn.signal.center))
        return inner(*a, **k)
    sn._ppseq_to_bits = counted
    if qad0 is not None:
        demod = sn.signal.quad_demod

        def forced():
            q = demod()
            if len(q) > 2:
                q[0] = qad0
            return q
        sn.signal.quad_demod = forced
    rec = {k: [] for k in ("above", "noise", "noise_type", "pause", "index", "n_msg")}
    updates, a = 0, 0
    for c in lens:
        c = int(c)
        before = sn.signal.noise_threshold
        sn._ProtocolSniffer__demodulate_data(iq[a:a + c])       # what rcv_device.data[a:b] hands over: the raw (n, 2) array (IQArray.py:22-23)
        a += c
        after = sn.signal.noise_threshold
        updates += (after != before) or (type(after) is not type(before))
        rec["above"].append(-1 if c == 0 else int(sn.pause_length == 0))
        rec["noise"].append(float(after))
        rec["noise_type"].append(type(after).__name__)
        rec["pause"].append(int(sn.pause_length))
        rec["index"].append(int(sn._ProtocolSniffer__current_buffer_index))
        rec["n_msg"].append(len(sn.messages))
    msgs = sn.messages
    assert len(msgs) >= min_msgs and len(flushes) >= 1, (name, len(msgs), len(flushes))
    if adaptive:
        assert updates >= 1, name
    if want_trim:
        assert log.trims >= 1, name
    bits = np.concatenate([np.asarray(m.plain_bits, np.uint8) for m in msgs]) if msgs else np.zeros(0, np.uint8)
    msg_off = np.cumsum([0] + [len(m.plain_bits) for m in msgs]).astype(np.int64)
    ts = np.asarray([m.timestamp for m in msgs], np.float64)
    # (Message does not keep the first bit's sample position: FIRST_POS records it from what _ppseq_to_bits returned inside the flush)
    out = dict(iq=iq, chunk_lens=np.asarray(lens, np.int64), modulation_type=mod, samples_per_symbol=sps, bits_per_symbol=bps,
               center=np.float64(center), center_spacing=np.float64(spacing), noise_threshold=np.float64(noise), tolerance=tolerance,
               adaptive_noise=bool(adaptive), automatic_center=bool(autocenter), buffer_samples=int(buffer_mb * 1000 * 1000 / 8),
               sample_rate=np.float64(SAMPLE_RATE), clock=np.float64(CLOCK),
               rec_above=np.asarray(rec["above"], np.int8), rec_noise=np.asarray(rec["noise"], np.float64),
               rec_noise_type=np.asarray(rec["noise_type"]), rec_pause=np.asarray(rec["pause"], np.int64),
               rec_index=np.asarray(rec["index"], np.int64), rec_n_msg=np.asarray(rec["n_msg"], np.int64),
               centers=np.asarray(flushes, np.float64), bits=bits, msg_off=msg_off,
               pauses=np.asarray([m.pause for m in msgs], np.int64), first_pos=np.asarray(FIRST_POS, np.int64),
               timestamps=ts, timestamps_minus_clock=ts - CLOCK, n_trims=log.trims)
    assert len(FIRST_POS) == len(msgs), name
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: rows={len(iq)} chunks={len(lens)} flushes={len(flushes)} msgs={len(msgs)} bits={[len(m.plain_bits) for m in msgs]} "
          f"noise_updates={updates} final_noise={rec['noise'][-1]!r}:{rec['noise_type'][-1]} trims={log.trims} bytes={os.path.getsize(path)}")
    assert os.path.getsize(path) < 480 * 1024, name
    FIRST_POS.clear()
    return out


# bit_sample_pos[i][0] of every message, taken from what the reference's own _ppseq_to_bits returns inside the flush
FIRST_POS = []
_inner_ppseq = ProtocolAnalyzer._ppseq_to_bits


def _recording_ppseq(self, *a, **k):
    res = _inner_ppseq(self, *a, **k)
    FIRST_POS.extend(int(p[0]) for p in res[2])
    return res


ProtocolAnalyzer._ppseq_to_bits = _recording_ppseq


def main():
    os.makedirs(OUT, exist_ok=True)
    f32 = np.float32
    # automatic center: the capture starts inside a burst.  Leading noise alone is appended for 10 symbols and then flushed by itself,
    # detect_center finds nothing in it and the reference fails in grab_pulse_lens(center=None) -- not a case a fixture can pin
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=1, lead=0)
    run_case("fsk_f32_adaptive_autocenter", iq, chunk_lengths(len(iq), 150, 900, 11), "FSK", 100, noise=0.1, adaptive=True, autocenter=True)
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=2, dtype=np.int8)
    run_case("fsk_i8_adaptive", iq, chunk_lengths(len(iq), 150, 900, 12), "FSK", 100, noise=10.0, adaptive=True)
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=3, dtype=np.int16)
    run_case("fsk_i16_adaptive", iq, chunk_lengths(len(iq), 150, 900, 13), "FSK", 100, noise=3000.0, adaptive=True)
    # unsigned captures: the reference's gate does not remove the offset, so pause and burst both have a large RMS per component; it
    # decodes such captures poorly -- the fixtures pin that behaviour as it is
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=4, dtype=np.uint8)
    run_case("fsk_u8", iq, chunk_lengths(len(iq), 150, 900, 14), "FSK", 100, noise=132.0, min_msgs=1)
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=5, dtype=np.uint16)
    run_case("fsk_u16", iq, chunk_lengths(len(iq), 150, 900, 15), "FSK", 100, noise=33500.0, min_msgs=1)
    iq = capture("ASK", 1, 100, 4, 64, 2500, seed=6, lead=0)
    run_case("ask_f32_autocenter", iq, chunk_lengths(len(iq), 150, 900, 16), "ASK", 100, center=0.3, noise=0.1, autocenter=True)
    iq = capture("PSK", 1, 100, 4, 64, 2500, seed=7)
    run_case("psk_f32", iq, chunk_lengths(len(iq), 150, 900, 17), "PSK", 100, noise=0.1)
    iq = capture("FSK", 2, 100, 4, 128, 2500, seed=8)
    run_case("fsk4_f32", iq, chunk_lengths(len(iq), 150, 900, 18), "FSK", 100, bps=2, spacing=0.1, noise=0.1)
    # 0.02 MB = 2500 rows: every burst overruns the buffer (trimmed append, then the full-buffer flush)
    iq = capture("FSK", 1, 100, 4, 64, 2500, seed=9)
    run_case("fsk_f32_small_buffer", iq, chunk_lengths(len(iq), 150, 900, 19), "FSK", 100, noise=0.1, buffer_mb=0.02, want_trim=True)
    # chunks shorter than 8 rows (numpy's pairwise sum takes its plain loop below 8 elements) and empty chunks
    iq = capture("FSK", 1, 100, 3, 64, 2500, seed=10)
    head = [0, 1, 2, 3, 4, 5, 6, 7, 0] + [int(v) for v in np.random.default_rng(20).integers(1, 8, 1500)]
    lens = chunk_lengths(len(iq), 150, 900, 20, head=head)
    lens = np.concatenate([lens[:-3], [0], lens[-3:]])
    run_case("fsk_f32_tiny_chunks", iq, lens, "FSK", 100, noise=0.1, adaptive=True)


if __name__ == "__main__":
    main()
