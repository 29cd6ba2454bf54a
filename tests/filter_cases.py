"""Seeded inputs for the filter kernels (urh_amd/csrc/filters.hip) at the shapes and values its first tests left out; shared by
tests/test_filters_host.py (oracle against the real reference and its recorded outputs) and tests/test_filters_gpu.py (kernels against
the oracle).  numpy only; nothing outside the repository is read.  DESIGN.md 7.11 has the notes.

Families: A tap counts (the reference's own presets, the LDS thresholds of launch_fir), B the checked kernel behind the fast one,
C the fused chunk statistics, D IIR sizes and values, E empty taps."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "filter", "edges.npz")

# ---- geometry of the FIR kernels (filters.hip:36-38) ---------------------------------------------------------------------------------------
FIR_R = 8                      # kFirR: outputs per lane
TILE = 256 * FIR_R             # kFirTile: outputs per workgroup
N3 = 2 * TILE + 5              # three tiles, the last one partial
LDS_PLAIN = 64 * 1024          # fir_lds_attr (filters.hip:449): above it hipFuncSetAttribute raises the kernel's dynamic LDS limit
LDS_REFUSED = 150 * 1024       # launch_fir (filters.hip:468): above it URHGPU_ERR_UNSUPPORTED
SAFE = np.float32(2.0 ** 60)   # kFirSafeBits (filters.hip:63): a tile with a component at or above it goes to the checked kernel


def fir_lds_bytes(m: int) -> int:
    """dynamic LDS of k_fir for m taps (launch_fir, filters.hip:466-467): taps, staged history + tile, one pad per 8 samples"""
    hist = ((m - 1) // FIR_R) * FIR_R + FIR_R - 1
    return (((m + 1) & ~1) + (hist + TILE) + ((hist + TILE) >> 3) + 1) * 8


def fir_fast_lds_bytes(m: int) -> int:
    """dynamic LDS of k_fir_fast for m taps (launch_fir, filters.hip:475-476): rows of 8 samples + 1 pad"""
    m_pad = ((m - 1) // FIR_R) * FIR_R + FIR_R
    return ((m_pad + TILE) // FIR_R) * (FIR_R + 1) * 8


def last_m(bytes_of, limit: int) -> int:
    """the largest tap count whose LDS need is at most `limit` (the need never falls as m grows)"""
    m = 1
    while bytes_of(m + 1) <= limit:
        m += 1
    return m


M_CHECKED_PLAIN = last_m(fir_lds_bytes, LDS_PLAIN)          # 2768: from 2769 taps k_fir needs the raised limit
M_FAST_PLAIN = last_m(fir_fast_lds_bytes, LDS_PLAIN)        # 5232: from 5233 taps k_fir_fast needs it too
M_MAX = last_m(fir_lds_bytes, LDS_REFUSED)                  # 7950: 7951 taps are refused
RANDOM_TAP_COUNTS = (M_CHECKED_PLAIN, M_CHECKED_PLAIN + 1, M_FAST_PLAIN, M_FAST_PLAIN + 1, M_MAX)
PRESET_LENGTHS = {"Very Narrow": 4001, "Narrow": 401, "Medium": 51, "Wide": 41, "Very Wide": 11}


def noise(rng, n, scale=1.0) -> np.ndarray:
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


def same_bits(a, b) -> bool:
    """complex64 arrays equal bit for bit, a NaN part equal to a NaN part"""
    a, b = np.ascontiguousarray(a, np.complex64), np.ascontiguousarray(b, np.complex64)
    if a.shape != b.shape:
        return False
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    return bool(((ua == ub) | (np.isnan(ua.view(np.float32)) & np.isnan(ub.view(np.float32)))).all())


# ---- A: tap counts -------------------------------------------------------------------------------------------------------------------------
def preset_taps(name: str) -> np.ndarray:
    """the taps the reference designs for one of Filter.BANDWIDTHS, as its FIR receives them (complex64)"""
    from urh_amd.filter import Filter, bandpass_taps
    return np.ascontiguousarray(bandpass_taps(-0.1, 0.2, Filter.BANDWIDTHS[name]), dtype=np.complex64)


def a_cases():
    """[(name, samples, taps)]: every preset and every threshold count on three tiles, the longest preset also on a capture shorter than it"""
    rng = np.random.default_rng(7_11_01)
    out = []
    for name in PRESET_LENGTHS:
        out.append(("preset_" + name.replace(" ", "_"), noise(rng, N3), preset_taps(name)))
    out.append(a_golden_case())
    for m in RANDOM_TAP_COUNTS:
        out.append((f"random_{m}", noise(rng, N3), noise(rng, m, 0.05)))
    return out


def a_golden_case():
    """4001 taps on 1000 samples: the filter is longer than the capture (recorded from the reference)"""
    rng = np.random.default_rng(7_11_02)
    return "preset_Very_Narrow_n1000", noise(rng, 1000), preset_taps("Very Narrow")


def a_halo_cases():
    """[(name, capture, taps, cut)]: the shard capture[cut:] with capture[cut - (m - 1):cut] as its halo; cut is no multiple of 8"""
    rng = np.random.default_rng(7_11_03)
    out = []
    for name, cut in (("Narrow", 403), ("Very Narrow", 4003)):
        h = preset_taps(name)
        assert cut % 8 and cut >= len(h) - 1
        out.append(("halo_" + name.replace(" ", "_"), noise(rng, cut + N3), h, cut))
    return out


def a_sequence():
    """three calls on one context: small, the largest accepted filter on three tiles, small again"""
    rng = np.random.default_rng(7_11_04)
    return [(noise(rng, 100), noise(rng, 3)), (noise(rng, N3), noise(rng, M_MAX, 0.05)), (noise(rng, 100), noise(rng, 3))]


# ---- B: the checked kernel behind the fast one ---------------------------------------------------------------------------------------------
B_TILES = 1025                  # k_fir works the list off with at most 1024 workgroups (launch_fir, filters.hip:485)


def b_every_tile():
    """an infinite tap hands every tile back: 1026 tiles, so the grid-stride loop over the list makes a second trip"""
    rng = np.random.default_rng(7_11_05)
    h = np.array([0.5 - 0.25j, np.inf, 0.125 + 1j], dtype=np.complex64)
    return noise(rng, B_TILES * TILE + 9), h


def b_halo_tile0():
    """(halo, shard, taps): 64 taps, three tiles; the halo's last samples are not finite or huge, so tile 0 alone is handed back"""
    rng = np.random.default_rng(7_11_06)
    m = 64
    halo, x, h = noise(rng, m - 1), noise(rng, N3), noise(rng, m, 0.125)
    halo[-3:] = np.array([np.nan, np.inf, 1e30], dtype=np.complex64)
    return halo, x, h


def b_threshold(at: bool):
    """300 equal real taps and 700 equal real samples: just below 2^60 (stays in the fast kernel) or exactly 2^60 (handed back)"""
    v = SAFE if at else np.nextafter(SAFE, np.float32(0))
    return np.full(700, v, dtype=np.complex64), np.full(300, v, dtype=np.complex64)


# ---- C: fused chunk statistics -------------------------------------------------------------------------------------------------------------
C_N, C_M = 5 * TILE + 777, 64
C_GEOMETRIES = ((2048, 5), (2049, 5), (3000, 3), (3000, 2), (11017, 1))       # (chunk, n_chunks); chunk k = [n - (k+1) chunk, n - k chunk)
C_VARIANTS = ("plain", "nan", "huge")


def c_case(chunk: int, n_chunks: int, variant: str, with_halo: bool):
    """(halo or None, samples, taps).  A loud front and a quiet end, so that detect_noise_level's decision has chunks to choose from.
    nan: one NaN sample 30 before the last chunk boundary (its 64 NaN outputs lie on both sides); with one chunk, across a tile boundary.
    huge: a 3e24 sample just behind that boundary: its tile is handed to the checked kernel and straddles two chunks."""
    assert C_N == 11017 and chunk >= TILE and n_chunks * chunk <= C_N
    rng = np.random.default_rng([7_11_07, chunk, n_chunks, C_VARIANTS.index(variant), int(with_halo)])
    x = noise(rng, C_N)
    x[C_N * 2 // 3:] *= np.float32(0.03)
    h = noise(rng, C_M, 0.125)
    halo = noise(rng, C_M - 1) if with_halo else None
    boundary = C_N - chunk if n_chunks > 1 else 2 * TILE
    if variant == "nan":
        x[boundary - 30] = np.nan
    elif variant == "huge":
        x[boundary + 5] = np.float32(3e24)
    return halo, x, h


def c_reference(oracle, halo, x, h, chunk, n_chunks):
    """(filtered, [magnitudes of chunk k]) by the oracle; with a halo: the same stretch of the one-pass result on halo + samples"""
    if halo is None:
        y = oracle.fir_filter(x, h)
    else:
        y = oracle.fir_filter(np.concatenate([halo, x]), h)[len(halo):]
    mags = oracle.get_magnitudes(np.ascontiguousarray(y).view(np.float32).reshape(-1, 2))
    n = len(x)
    return y, [mags[n - (k + 1) * chunk:n - k * chunk] for k in range(n_chunks)]


def sum_bound(chunk_mags) -> float:
    """chunk * 2^-52 * fsum: twice the first-order worst case (n - 1) u sum|x|, u = 2^-53, of ANY order of adding `chunk` non-negative doubles"""
    return len(chunk_mags) * 2.0 ** -52 * math.fsum(chunk_mags)


# ---- D: IIR --------------------------------------------------------------------------------------------------------------------------------
D_ORDERS = ((0, 0), (0, 2), (1, 0), (3, 2), (2, 4))                           # (M feed-forward, N feedback)
D_LONG, D_PERIOD = 4097, 61
D_FINITE = [complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0), complex(1e-40, -1e-40), complex(1, -1), complex(-1, 1),
            complex(3e38, -3e38), complex(-3e38, 3e38)]
D_WILD = D_FINITE + [complex(np.inf, np.inf), complex(-np.inf, np.inf), complex(np.inf, 1), complex(1, -np.inf), complex(np.nan, 0), complex(1, np.nan)]
D_COEFS = (0.0, -0.0, np.inf, np.nan)


def d_start(M: int, N: int) -> int:
    return max(M, N + 1)


def d_sizes(M: int, N: int):
    s = d_start(M, N)
    return sorted({1, s - 1, s, s + 1, D_LONG})


def _d_samples(rng, n, values, late: bool):
    """finite noise -- for the long size a pattern of period 61 (coprime with every block and wave size), which keeps the recorded outputs small --
    with `values` at seeded positions; late: in the last quarter only, so that a feedback filter has finite outputs in front of them"""
    base = noise(rng, min(n, D_PERIOD))
    x = np.resize(base, n).astype(np.complex64) if n else base[:0]
    k = min(n, max(len(values), n // 128))
    lo = n * 3 // 4 if late and n > 64 else 0
    pos = rng.choice(np.arange(lo, n), size=min(k, n - lo), replace=False) if n else np.zeros(0, np.int64)
    for i, p in enumerate(pos):
        x[p] = np.complex64(values[i % len(values)] if n > len(values) else values[int(rng.integers(len(values)))])
    return x


def d_cases():
    """[(name, a, b, x)] -- a, b float64; x complex64"""
    out = []
    x0 = noise(np.random.default_rng(7_11_08), 12)
    x0[4], x0[8] = complex(np.inf, np.inf), complex(-np.inf, np.inf)
    out.append(("annexg_ff", np.array([0.5]), np.zeros(0), x0))
    out.append(("annexg_fb", np.array([0.5, 0.25]), np.array([0.125]), x0.copy()))
    for M, N in D_ORDERS:
        for n in d_sizes(M, N):
            for kind, values in (("finite", D_FINITE), ("wild", D_WILD)):
                rng = np.random.default_rng([7_11_09, M, N, n, len(values)])
                a, b = rng.standard_normal(M) * 0.3, rng.standard_normal(N) * 0.2
                out.append((f"m{M}_n{N}_len{n}_{kind}", a, b, _d_samples(rng, n, values, late=kind == "wild")))
        # one coefficient at a time 0.0, -0.0, inf, nan: the first feed-forward one, the last feedback one
        for n in (d_start(M, N) + 1,) + ((D_LONG,) if (M, N) == (3, 2) else ()):
            for ci, c in enumerate(D_COEFS):
                for where in ("a", "b"):
                    if (where == "a" and M == 0) or (where == "b" and N == 0):
                        continue
                    rng = np.random.default_rng([7_11_10, M, N, n, ci, where == "a"])
                    a, b = rng.standard_normal(M) * 0.3, rng.standard_normal(N) * 0.2
                    if where == "a":
                        a[0] = c
                    else:
                        b[-1] = c
                    out.append((f"m{M}_n{N}_len{n}_{where}{['p0', 'n0', 'inf', 'nan'][ci]}", a, b, _d_samples(rng, n, D_FINITE, late=False)))
    rng = np.random.default_rng(7_11_11)
    out.append(("grows_past_float32", np.array([0.5]), np.array([1.5]), noise(rng, 400)))
    return out


# ---- E: empty taps -------------------------------------------------------------------------------------------------------------------------
def e_cases():
    """[(name, samples, taps)]; the reference gives N - 1 zeros, ValueError, an empty array"""
    x = noise(np.random.default_rng(7_11_12), 5)
    return [("n5_m0", x, np.zeros(0, np.complex64)), ("n0_m0", x[:0], np.zeros(0, np.complex64)), ("n0_m3", x[:0], noise(np.random.default_rng(1), 3))]


def fir_outcome(fir, x, h):
    """("array", result) or ("ValueError", None)"""
    try:
        return "array", np.asarray(fir(x, h))
    except ValueError:
        return "ValueError", None


# ---- the recorded outputs of the real reference (tests/golden/make_filter_edges_golden.py) -----------------------------------------------
def golden_fir_cases():
    """the FIR cases that are recorded: [(name, samples, taps)]"""
    return [a_golden_case(), ("threshold_below", *b_threshold(False)), ("threshold_at", *b_threshold(True))]


def pack(arrays, dtype):
    """(flat, offsets) of a list of 1-D arrays: the file holds a handful of entries, not four per case"""
    off = np.cumsum([0] + [len(a) for a in arrays]).astype(np.int64)
    flat = np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays]) if arrays else np.zeros(0, dtype)
    return flat.astype(dtype), off


def unpack(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def load_golden():
    """{"fir": {name: (x, h, y)}, "iir": {name: (a, b, x, y)}, "empty": {name: (x, h, kind, y or None)}}"""
    z = np.load(GOLDEN, allow_pickle=False)
    g = {"fir": {}, "iir": {}, "empty": {}}
    for sec, keys in (("fir", "xhy"), ("iir", "abxy"), ("empty", "xhy")):
        cols = [unpack(z[f"{sec}_{k}"], z[f"{sec}_{k}_off"]) for k in keys]
        for i, name in enumerate(str(s) for s in z[sec + "_names"]):
            g[sec][name] = tuple(c[i] for c in cols)
    for i, name in enumerate(str(s) for s in z["empty_names"]):
        x, h, y = g["empty"][name]
        kind = str(z["empty_kind"][i])
        g["empty"][name] = (x, h, kind, y if kind == "array" else None)
    return g
