"""numpy model of k_noise_decide (urh_amd/csrc/filters.hip): the decision part of AutoInterpretation.detect_noise_level
(AutoInterpretation.py:74-91) on the per-chunk (sum, max) of the magnitudes, chunk 0 = the capture's LAST chunk, with every scalar
type spelled out -- what the kernel computes, statement for statement -- and the flag protocol of include/urhgpu.h
(urhgpu_noise_result).  test_auto_noise_host.py pins it against the oracle's detect_noise_level and against the real reference's
thresholds in tests/golden/auto_noise.json; test_auto_noise_gpu.py compares the device with the oracle directly."""
import math

import numpy as np

FLAG_RAISES, FLAG_OK, FLAG_GATES_ALL = 0, 1, 2


def max_magnitude(dtype) -> float:
    """Signal.max_magnitude (Signal.py:404-406) with IQArray.min_max_for_dtype's bounds"""
    dtype = np.dtype(dtype)
    lo, hi = (-1, 1) if dtype.kind == "f" else (int(np.iinfo(dtype).min), int(np.iinfo(dtype).max))
    return (2 * max(lo ** 2, hi ** 2)) ** 0.5


def chunk_geometry(n: int):
    """(chunk, n_chunks): chunks of max(1, int(n / 100)) samples counted from the END of the capture; none for n <= 3 (:61-72)"""
    if n <= 3:
        return 1, 0
    chunk = max(1, int(n * 1 / 100))
    return chunk, n // chunk


def chunk_stats(magnitudes, n=None):
    """(sums, maxs, chunk) in float64, chunk 0 = the last one: what urhgpu_magnitude_chunk_stats_dev hands k_noise_decide"""
    m = np.asarray(magnitudes, dtype=np.float64)
    n = len(m) if n is None else n
    chunk, k = chunk_geometry(n)
    if k == 0:
        return np.zeros(0), np.zeros(0), chunk
    # (np.add.reduce over the contiguous chunk: the sum np.mean divides, so sums / chunk IS np.mean bit for bit)
    parts = [np.ascontiguousarray(m[n - (j + 1) * chunk:n - j * chunk]) for j in range(k)]
    return np.array([np.add.reduce(c) for c in parts]), np.array([np.max(c) for c in parts]), chunk


def decide(sums, maxs, chunk: int, max_mag: float):
    """k_noise_decide: (noise as a Python float, flag, n_candidates, min_mean, max_mean).  Every operation in the type the kernel uses."""
    sums, maxs = np.asarray(sums, dtype=np.float64), np.asarray(maxs, dtype=np.float64)
    k = len(sums)
    noise, flag, cand, lo, hi = 0.0, FLAG_OK, 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        if k > 0:
            means = (sums / np.float64(chunk)).astype(np.float32)          # a double division rounded to float32
            mn, mx, nan = means[0], means[0], bool(means[0] != means[0])
            for e in means[1:]:                                            # util.minmax's comparisons
                nan = nan or bool(e != e)
                if e > mx:
                    mx = e
                if e < mn:
                    mn = e
            lo, hi = float(mn), float(mx)                                  # Python floats: doubles
            # a NaN mean: np.min is NaN, no chunk compares, np.max([]) raises ValueError, detect_noise_level returns 0
            if not nan and not (hi == 0.0 or lo / hi > 0.9):
                lim = np.float32(1.1) * mn                                 # float32 product (a float32 scalar times a Python float)
                assert lim.dtype == np.float32
                result, res_nan = 0.0, False
                for j in range(k):
                    if not (means[j] <= lim):
                        continue
                    m = float(maxs[j])
                    res_nan = res_nan or m != m
                    if cand == 0 or m > result:
                        result = m
                    cand += 1
                if cand > 0:
                    if res_nan:
                        result = math.nan
                    if result != result or math.isinf(result):
                        noise, flag = result, FLAG_RAISES
                    else:
                        noise = float(np.ceil(np.float64(result) * np.float64(10000.0)) / np.float64(10000.0))
    if flag == FLAG_OK and not (noise < max_mag):
        flag = FLAG_GATES_ALL
    return noise, flag, cand, lo, hi


def detect(magnitudes, dtype):
    """(noise, flag) for a capture's magnitudes (util.get_magnitudes: float64)"""
    sums, maxs, chunk = chunk_stats(magnitudes)
    noise, flag, _, _, _ = decide(sums, maxs, chunk, max_magnitude(dtype))
    return noise, flag


def block_values(noise, flag, configured: float, in_pass: bool):
    """(noise_f32, noise_sqrd) of the result block: (float)noise and its fp32 square -- afp_demod's `float noise_mag` argument and
    noise_mag * noise_mag --, or the configured threshold's where a pass does not use the value (flag 0, 2)"""
    f = np.float32(configured) if (in_pass and flag != FLAG_OK) else np.float32(noise)
    return f, np.float32(f * f)
