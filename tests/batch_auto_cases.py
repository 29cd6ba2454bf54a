"""Shared by the tests of a batch with an automatic noise threshold per capture (test_batch_auto_host.py, test_batch_auto_gpu.py) and by
tests/golden/make_batch_auto_golden.py: the size sweep and the flag captures, built from tests/noise_cases.py's seeded recipe."""
import json
import os

import numpy as np

import noise_cases as nc

# no chunks | chunk 1 against 2 | 199 against 100 chunks | a dropped front remainder | chunk 7 | 8 (the sequential sum meets the eight
# accumulators) | chunk 127 | 128 | 129 (one leaf meets a split) | the longest capture a batch takes
SWEEP_LENGTHS = (0, 1, 3, 4, 5, 99, 100, 101, 199, 200, 201, 799, 800, 801, 900, 12_799, 12_800, 12_801, 12_927, 25_700, 65_537, 196_607)
# captures of the sweep with a non-zero threshold, per sample type (the oracle's detect_noise_level; uint16: wrapped sums give NaN means)
SWEEP_NONZERO = {"float32": 19, "int16": 19, "int8": 13, "uint8": 7, "uint16": 0}
N_FLAGS = 6000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_auto", "batch_auto.json")


def sweep(dtype):
    """the 22 captures of the size sweep for a sample type: gains cycled over STREAM_GAINS"""
    out = []
    for i, n in enumerate(SWEEP_LENGTHS):
        sigma, amp = nc.STREAM_GAINS[i % 8]
        out.append(nc.capture(7000 + i, n, dtype=np.dtype(dtype), sigma=sigma, amp=amp))
    return out


def flag_captures_f32():
    """float32, n = 6000: (name, capture) in the batch's order -- clean, all zeros, constant envelope, one NaN sample, +inf at every 50th
    sample's I, a threshold that gates everything, the clean capture again"""
    n = N_FLAGS
    clean = nc.capture(7100, n, sigma=0.01, amp=0.5)
    one_nan = np.array(nc.capture(7101, n, sigma=0.01, amp=0.5))
    one_nan[n // 2, 1] = np.nan
    infs = np.array(nc.capture(7102, n, sigma=0.01, amp=0.5))
    infs[::50, 0] = np.inf
    return [("clean", clean), ("zeros", np.zeros((n, 2), np.float32)), ("constant", nc.constant_envelope(n)), ("one-nan", one_nan),
            ("inf", infs), ("gates-all", nc.capture(4000, n, sigma=1.5, amp=3.0)), ("clean-again", clean)]


def flag_captures_i8():
    """int8, n = 6000: clean, the capture whose threshold is not below max_magnitude (181.0194 against 181.0193...), clean again"""
    n = N_FLAGS
    clean = nc.capture(7100, n, dtype=np.int8, sigma=0.01, amp=0.5)
    return [("clean", clean), ("gates-all", nc.capture(4000, n, dtype=np.int8, sigma=1.5, amp=3.0)), ("clean-again", clean)]


def load_golden():
    with open(GOLDEN) as fh:
        return json.load(fh)
