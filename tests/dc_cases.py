"""Inputs of the DC-correction tests, shared by the host model (test_dc_correction_host.py) and the GPU (test_dc_correction_gpu.py),
and the reference they are compared with: numpy's own expression, evaluated once per input.

CHUNK is the length of a speculated chunk of the float32 sum (urh_amd/csrc/dc_correct.hip); the cases place their
events relative to its seams."""
import functools

import numpy as np

CHUNK = 4096
SIZES = (100_003, 300_007)
INT_DTYPES = (np.int8, np.uint8, np.int16, np.uint16)
B24 = np.float32(2.0 ** 24)


def numpy_dc(x):
    """(x - mean, mean) as the reference computes them (Filter.py:31-35): np.mean(x, axis=0) and the subtraction; for integer captures
    the float64 difference is cast back into the sample type (what storing it into the IQArray / receive buffer does)."""
    with np.errstate(all="ignore"):
        mean = np.mean(x, axis=0)
        diff = x - mean
        out = diff if x.dtype == np.float32 else diff.astype(x.dtype)
    assert out.dtype == x.dtype
    return out, mean


def same_bits(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | nan))


def _noise(n, seed, amp=1.0, dc=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (amp * rng.uniform(-1.0, 1.0, (n, 2)) + np.asarray(dc)).astype(np.float32)


def _antisymmetric(n, seed):
    """noise whose every chunk is x, ..., -x mirrored: the exact mean is exactly zero and the running sum returns to (about) zero at every seam"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 2), np.float32)
    for a in range(0, n, CHUNK):
        m = min(CHUNK, n - a)
        h = rng.uniform(-1.0, 1.0, (m // 2, 2)).astype(np.float32)
        x[a:a + m // 2] = h
        x[a + m - m // 2:a + m] = -h[::-1]
    return x


def _zero_mean_spiked(n, seed):
    """_antisymmetric with (2^24, 1, -2^24, -1) at the head of every chunk: the exact mean is still exactly zero, but the sequential float32
    sum loses the +1 (2^24 + 1 is a tie that rounds to 2^24) and keeps the -1, so it is one further from the float64 guess at every seam, and
    every chunk's path runs from about zero up to 2^24 and back: no chunk behind the first can be derived from its speculation."""
    x = _antisymmetric(n, seed)
    for a in range(0, n, CHUNK):
        if n - a >= 8:
            x[a:a + 4] = np.array([[B24, -B24], [1, -1], [-B24, B24], [-1, 1]], np.float32)
            m = min(CHUNK, n - a)
            x[a + m - 4:a + m] = 0          # (the mirrored partners of the four overwritten samples)
    return x


def _crossing(n, shift):
    """Integers, so that every float32 sum is exact: the true sum of column I is one behind the float64 guess from sample 3 on (the 1 of
    2^24 + 1 is lost) and reaches 2^13 = 8192 -- a binade's edge -- `shift` samples in front of the seam at sample 8192 (negative: behind).
    Column Q is the same, negated."""
    x = np.ones((n, 2), np.float32)
    x[0, 0], x[1, 0], x[2, 0] = B24, 1.0, -B24
    x[3, 0] = 4.0 + shift                    # sum after sample i >= 3: i + 1 + shift  ->  8192 after sample 8191 - shift
    x[:, 1] = -x[:, 0]
    return x


def _ties(n, seed, odd):
    """the sum lives in [2^24, 2^25), u = 2; every term is 1 or 3: an odd multiple of u / 2, so every addition is an exact tie.  Entered with an
    even (2^23) or an odd (2^23 + 1) k."""
    rng = np.random.default_rng(seed)
    x = rng.choice(np.array([1.0, 3.0], np.float32), (n, 2))
    x[0] = B24 + (2.0 if odd else 0.0)
    x[1] = 2.0                               # (not a tie: the exact sum at a seam is then even, and half of it of either parity)
    x[:, 1] = -x[:, 1]
    return x


def _odd_guess(n, seed, with_ties):
    """2^23, then three times 0.25: each is lost by the float32 sum (u = 1) while the float64 sum keeps 0.75 and rounds to one unit more -- the
    guess of every later chunk is off by exactly one ulp.  The rest are small integers (exact in both), optionally with 0.5 (ties) among them."""
    rng = np.random.default_rng(seed)
    vals = [1.0, 2.0, 3.0] + ([0.5] if with_ties else [])
    x = rng.choice(np.array(vals, np.float32), (n, 2))
    x[0] = 2.0 ** 23
    x[1:4] = 0.25
    return x


def _special(n, kind, where):
    x = _noise(n, 11, 0.5, (0.25, -0.125))
    p = {"first": 0, "mid": n // 2 + 1, "seam": 3 * CHUNK, "last": n - 1}[where]
    if kind == "inf_minf":
        p = min(p, n - 2)
        x[p, 0], x[p + 1, 0] = np.inf, -np.inf
    else:
        x[p, 0] = {"nan": np.nan, "inf": np.inf}[kind]
    return x


def _overflow(n):
    x = _noise(n, 12, 0.5, (0.25, 0.25))
    x[n // 3, 0] = x[n // 3 + 1, 0] = 3e38
    x[n // 2, 1] = x[n // 2 + 1, 1] = -3e38
    x[CHUNK - 1, 1], x[CHUNK, 1] = 3e38, -3e38        # no overflow, but a sum of 3e38 across a seam
    return x


def _denormal(n, seed, dc):
    rng = np.random.default_rng(seed)
    k = rng.integers(-1000 + dc, 1001 + dc, (n, 2)).astype(np.float64)
    x = (k * 2.0 ** -149).astype(np.float32)
    assert np.all(np.abs(x) < np.finfo(np.float32).tiny)
    return x


F32_CASES = {
    "dc_10x_pos": lambda n: _noise(n, 1, 0.1, (1.0, 1.0)),
    "dc_10x_neg": lambda n: _noise(n, 2, 0.1, (-1.0, -1.0)),
    "dc_100th_pos": lambda n: _noise(n, 3, 1.0, (0.01, 0.01)),
    "dc_100th_neg": lambda n: _noise(n, 4, 1.0, (-0.01, -0.01)),
    "zero_mean": lambda n: _antisymmetric(n, 5),
    "zero_mean_spiked": lambda n: _zero_mean_spiked(n, 6),
    "sign_change": lambda n: np.concatenate([_noise(n // 2, 7, 0.1, (0.5, -0.5)), _noise(n - n // 2, 8, 0.1, (-1.0, 1.0))]),
    "cross_inside": lambda n: _crossing(n, 1000),
    "cross_on_seam": lambda n: _crossing(n, 0),
    "cross_before_seam": lambda n: _crossing(n, 1),
    "cross_after_seam": lambda n: _crossing(n, -1),
    "ties_even_k": lambda n: _ties(n, 9, False),
    "ties_odd_k": lambda n: _ties(n, 9, True),
    "odd_guess": lambda n: _odd_guess(n, 10, False),
    "odd_guess_ties": lambda n: _odd_guess(n, 10, True),
    **{f"{kind}_{where}": functools.partial(_special, kind=kind, where=where)
       for kind in ("nan", "inf", "inf_minf") for where in ("first", "mid", "seam", "last")},
    "overflow": _overflow,
    "denormal": lambda n: _denormal(n, 13, 0),
    "denormal_dc": lambda n: _denormal(n, 14, 900),
    "neg_zero": lambda n: np.full((n, 2), -0.0, np.float32),
}
# cases in which a DC term dominates: nearly every chunk must be derived from its speculation, not re-evaluated (see the GPU test)
TRANSLATED_CASES = ("dc_10x_pos", "dc_10x_neg", "dc_100th_pos", "dc_100th_neg", "odd_guess")


@functools.lru_cache(maxsize=None)
def f32_case(name, n):
    """(input, numpy's output, numpy's mean), computed once and read-only"""
    x = np.ascontiguousarray(F32_CASES[name](n), dtype=np.float32)
    assert x.shape == (n, 2)
    out, mean = numpy_dc(x)
    for a in (x, out, mean):
        a.setflags(write=False)
    return x, out, mean


def generic(dtype, n, seed=0):
    """a capture with a DC term for the size sweep"""
    rng = np.random.default_rng(1000 + seed + n)
    if np.dtype(dtype) == np.float32:
        return (0.5 * rng.uniform(-1, 1, (n, 2)) + (0.125, -0.0625)).astype(np.float32)
    info = np.iinfo(dtype)
    span = info.max - info.min
    lo, hi = info.min + span // 8, info.max - span // 3          # off-centre: a DC term of its own
    return rng.integers(lo, hi + 1, (n, 2)).astype(dtype)


def int_cases(n=20_001):
    i8 = np.empty((n, 2), np.int8); i8[0::2] = -128; i8[1::2] = 127
    rng = np.random.default_rng(21)
    u8 = rng.integers(118, 139, (n, 2)).astype(np.uint8)
    u16 = rng.integers(0, 65536, (n, 2)).astype(np.uint16); u16[:, 1] = rng.integers(30000, 30020, n)
    i16 = rng.choice(np.array([-32768, 32767], np.int16), (n, 2)); i16[: n // 3, 1] = -32768; i16[n // 3:, 1] = 32767
    return {"int8_alternating": i8, "uint8_around_128": u8, "uint16_wrap": u16, "int16_extremes": i16}


def redo_bound(n):
    """Chunks (both columns) a DC-dominated capture may re-evaluate.  Its running sum moves away from zero through one binade after the other:
    behind the first chunk (entered exactly as guessed) there are at most ceil(log2(n_chunks)) edges, an edge spoils the chunk it falls in and,
    when it falls near that chunk's end, the margin of the next; three more per column for the first chunks of a weak DC term, whose sum
    the noise still moves across edges and through zero."""
    n_chunks = -(-n // CHUNK)
    return 2 * (2 * int(np.ceil(np.log2(n_chunks))) + 3)
