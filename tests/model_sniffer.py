"""Numpy engine for urh_amd.sniffer.LiveSniffer: the same engine interface as GpuSniffEngine, with the statistics written as the
reference's numpy expressions (ProtocolSniffer.py:213-220) and the flush going through the oracle.  It lets the sniffer's state
machine be checked against the reference's recorded runs without a GPU, and shows what the GPU engine has to reproduce.
TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

import urh_oracle as oracle
from urh_amd.sniffer import max_magnitude, trimmed_rows

SNIFFER_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sniffer")
SNIFFER_CASES = sorted(f[:-4] for f in os.listdir(SNIFFER_DIR) if f.endswith(".npz")) if os.path.isdir(SNIFFER_DIR) else []


def load_case(name):
    z = np.load(os.path.join(SNIFFER_DIR, name + ".npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["modulation_type"] = str(g["modulation_type"])
    for k in ("samples_per_symbol", "bits_per_symbol", "tolerance", "buffer_samples", "n_trims"):
        g[k] = int(g[k])
    for k in ("center", "center_spacing", "noise_threshold", "sample_rate", "clock"):
        g[k] = float(g[k])
    for k in ("adaptive_noise", "automatic_center"):
        g[k] = bool(g[k])
    return g


def chunks_of(g):
    a = 0
    for c in g["chunk_lens"]:
        yield g["iq"][a:a + int(c)]
        a += int(c)


class NumpySniffEngine:
    def __init__(self, dtype, buffer_samples):
        self.dtype = np.dtype(dtype)
        self.buffer = np.zeros((int(buffer_samples), 2), self.dtype)

    def stats_append(self, chunk, index):
        n = trimmed_rows(len(chunk), index, len(self.buffer))
        self.buffer[index:index + n] = chunk[:n]
        with np.errstate(all="ignore"):
            power_spectrum = chunk.real ** 2.0 + chunk.imag ** 2.0                 # :213
            # np.mean = np.add.reduce / count in the array's float type; the sniffer divides, the engine hands over the sum
            return np.add.reduce(power_spectrum, axis=None), np.max(power_spectrum)

    def flush(self, index, p, automatic_center):
        iq = np.ascontiguousarray(self.buffer[:index])
        if p.noise_threshold < max_magnitude(self.dtype):                        # Signal.quad_demod (Signal.py:474-484)
            qad = oracle.afp_demod(iq, p.noise_threshold, p.modulation_type, 2 ** p.bits_per_symbol, p.costas_loop_bandwidth)
            if p.modulation_type == "PSK" and len(qad) > 2:
                qad[0] = -4.0           # the sample costa_demod never writes: the library's documented value (include/urhgpu.h), as the fixtures
        else:
            qad = np.zeros(2, dtype=np.float32)
        center = p.center
        if automatic_center:
            center = oracle.detect_center(qad, max_size=150 * p.samples_per_symbol)
        pp = oracle.grab_pulse_lens(qad, center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
        return (center,) + tuple(oracle.ppseq_to_bits(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold))


def make_sniffer(g, engine, pipe=None):
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import LiveSniffer
    p = DemodParams(g["modulation_type"], g["bits_per_symbol"], g["noise_threshold"], g["center"], g["center_spacing"], g["tolerance"],
                    g["samples_per_symbol"], 0.1, 8, True)
    return LiveSniffer(pipe, p, dtype=g["iq"].dtype, sample_rate=g["sample_rate"], adaptive_noise=g["adaptive_noise"],
                       automatic_center=g["automatic_center"], buffer_samples=g["buffer_samples"], clock=lambda: g["clock"],
                       engine=engine, trace=True)


def check_against_fixture(g, sniffer, chunks):
    """feed every chunk; every per-chunk record and every message must EQUAL what the reference recorded"""
    n_seen = 0
    for i, chunk in enumerate(chunks):
        new = sniffer.feed(chunk)
        t = sniffer.trace[-1]
        where = f"chunk {i}"
        above = -1 if t["above"] is None else int(t["above"])
        assert above == int(g["rec_above"][i]), where
        assert type(t["noise"]).__name__ == str(g["rec_noise_type"][i]), (where, type(t["noise"]).__name__, str(g["rec_noise_type"][i]))
        assert float(t["noise"]) == float(g["rec_noise"][i]), (where, float(t["noise"]), float(g["rec_noise"][i]))
        assert t["pause_length"] == int(g["rec_pause"][i]), where
        assert t["index"] == int(g["rec_index"][i]), where
        assert len(sniffer.messages) == int(g["rec_n_msg"][i]), where
        assert len(new) == len(sniffer.messages) - n_seen, where
        n_seen = len(sniffer.messages)
    assert len(sniffer.trace) == len(g["chunk_lens"])
    assert [float(c) for c in sniffer.centers] == [float(c) for c in g["centers"]]
    assert sniffer.center == (float(g["centers"][-1]) if len(g["centers"]) else g["center"])
    msgs = sniffer.messages
    assert len(msgs) == len(g["pauses"])
    for m, msg in enumerate(msgs):
        want = g["bits"][g["msg_off"][m]:g["msg_off"][m + 1]]
        assert np.array_equal(np.asarray(msg.plain_bits, np.uint8), want), f"message {m}: bits"
        assert msg.pause == int(g["pauses"][m]), f"message {m}: pause"
        assert msg.first_bit_sample_pos == int(g["first_pos"][m]), f"message {m}: first position"
        assert msg.timestamp == float(g["timestamps"][m]), f"message {m}: timestamp"
