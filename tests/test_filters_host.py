"""Pin the ORACLE's fir_filter / iir_filter on the inputs of tests/filter_cases.py before the kernels are judged against it
(tests/test_filters_gpu.py): against the real reference where oracle/_ref is built (every family), and against the reference's
recorded outputs (tests/golden/filter/edges.npz, tests/golden/make_filter_edges_golden.py) everywhere.  The builders' own conditions
are asserted here, and printed, so that no case passes vacuously.  No GPU needed."""
import os

import numpy as np
import pytest

import filter_cases as F


def _ref():
    import build_ref
    if not build_ref.built():
        pytest.skip("oracle/_ref not built (needs the reference)")
    return build_ref.import_ref()[0]


@pytest.fixture(scope="module")
def golden():
    return F.load_golden()


# ---- the builders --------------------------------------------------------------------------------------------------------------------------
def test_tap_counts_follow_the_lds_formulas():
    """the three thresholds are where launch_fir's formulas put them, and the presets have the lengths the reference designs"""
    assert (F.M_CHECKED_PLAIN, F.M_FAST_PLAIN, F.M_MAX) == (2768, 5232, 7950)
    assert F.fir_lds_bytes(2768) <= F.LDS_PLAIN < F.fir_lds_bytes(2769)
    assert F.fir_fast_lds_bytes(5232) <= F.LDS_PLAIN < F.fir_fast_lds_bytes(5233)
    assert F.fir_lds_bytes(7950) == 153_592 and F.fir_lds_bytes(7951) == 153_608 > F.LDS_REFUSED
    assert F.fir_lds_bytes(4001) == 86_512                       # the "Very Narrow" preset: k_fir above the plain limit on every call
    assert all(F.fir_lds_bytes(m + 1) >= F.fir_lds_bytes(m) and F.fir_fast_lds_bytes(m + 1) >= F.fir_fast_lds_bytes(m) for m in range(1, 8000))
    from urh_amd.filter import Filter, get_filter_length_from_bandwidth
    assert {k: get_filter_length_from_bandwidth(bw) for k, bw in Filter.BANDWIDTHS.items()} == F.PRESET_LENGTHS
    assert sorted(F.PRESET_LENGTHS.values()) == [11, 41, 51, 401, 4001]
    cases = F.a_cases()
    assert sorted(len(h) for _, _, h in cases) == sorted([11, 41, 51, 401, 4001, 4001, 2768, 2769, 5232, 5233, 7950])
    for name, x, h in cases:
        assert x.dtype == h.dtype == np.complex64 and np.isfinite(x.view(np.float32)).all() and np.isfinite(h.view(np.float32)).all(), name
        assert max(np.abs(x.view(np.float32)).max(), np.abs(h.view(np.float32)).max()) < F.SAFE, name      # all of it the fast kernel's
        assert len(x) in (F.N3, 1000) and F.N3 == 4101 and F.N3 % F.TILE
    assert [len(x) for name, x, h in cases if len(h) == 4001] == [F.N3, 1000]
    for name, x, h, cut in F.a_halo_cases():
        assert len(h) in (401, 4001) and cut % 8 and cut >= len(h) - 1 and len(x) - cut == F.N3, name
    seq = F.a_sequence()
    assert [(len(x), len(h)) for x, h in seq] == [(100, 3), (F.N3, 7950), (100, 3)]


def test_checked_kernel_cases_mean_what_they_say(oracle):
    x, h = F.b_every_tile()
    assert len(h) == 3 and np.isinf(h.view(np.float32)).sum() == 1 and np.isfinite(x.view(np.float32)).all()
    assert -(-len(x) // F.TILE) == 1026 > 1024 and len(x) % F.TILE == 9
    halo, xs, hs = F.b_halo_tile0()
    assert len(hs) == 64 and len(halo) == 63 and len(xs) == F.N3
    assert np.isnan(halo[-3].real) and np.isinf(halo[-2].real) and halo[-1].real == np.float32(1e30) >= F.SAFE
    assert np.isfinite(halo[:-3].view(np.float32)).all() and np.abs(xs.view(np.float32)).max() < F.SAFE      # tile 0 alone is handed back
    for at in (False, True):
        x, h = F.b_threshold(at)
        assert (len(x), len(h)) == (700, 300) and (x == x[0]).all() and (h == x[0]).all() and x[0].imag == 0
        assert (x[0].real >= F.SAFE) == at and np.nextafter(x[0].real, np.float32(np.inf)) >= F.SAFE
        with np.errstate(all="ignore"):
            y = oracle.fir_filter(x, h)
        inf = np.isinf(y.view(np.float32)).reshape(-1, 2)
        first = int(np.argmax(inf[:, 0]))
        print("threshold", "at" if at else "below", "first infinite output", first, "infinite", int(inf[:, 0].sum()))
        assert inf[:, 0].any() and not np.isnan(y.view(np.float32)).any() and inf[first:, 0].all()
        assert first == (255 if at else 256)                     # 256 terms of 2^120 are 2^128; one float below, the 257th term overflows
        assert (y.real[np.isinf(y.real)] > 0).all()


def test_statistics_cases_mean_what_they_say(oracle):
    """every geometry: chunk >= one tile, the NaN outputs on both sides of a boundary, the huge sample's tile on both sides of one, and a decision
    that is not the trivial 0 wherever there is more than one chunk"""
    from urh_amd.estimators import noise_level_from_chunk_stats
    assert F.C_N == 11017 == 5 * 2048 + 777 and F.C_M == 64
    assert F.C_GEOMETRIES == ((2048, 5), (2049, 5), (3000, 3), (3000, 2), (11017, 1))
    assert F.C_N - 2 * 3000 > 2 * F.TILE                       # (3000, 2): whole tiles in front of the first counted output
    for chunk, n_chunks in F.C_GEOMETRIES:
        for with_halo in (False, True):
            for variant in F.C_VARIANTS:
                halo, x, h = F.c_case(chunk, n_chunks, variant, with_halo)
                assert (halo is not None) == with_halo and len(x) == F.C_N and len(h) == 64
                with np.errstate(all="ignore"):
                    y, chunks = F.c_reference(oracle, halo, x, h, chunk, n_chunks)
                assert [len(c) for c in chunks] == [chunk] * n_chunks
                nan_out = np.nonzero(np.isnan(y.real))[0]
                if variant == "nan":
                    assert len(nan_out) == 64
                    if n_chunks > 1:
                        assert np.isnan(chunks[0]).any() and np.isnan(chunks[1]).any() and not any(np.isnan(c).any() for c in chunks[2:])
                    else:
                        assert nan_out[0] // F.TILE != nan_out[-1] // F.TILE
                else:
                    assert len(nan_out) == 0
                if variant == "huge":
                    p = int(np.argmax(np.abs(x.real)))
                    assert x[p].real == np.float32(3e24) >= F.SAFE
                    if n_chunks > 1:
                        b = F.C_N - chunk
                        assert p // F.TILE == b // F.TILE and p >= b > p // F.TILE * F.TILE        # the handed-back tile holds the boundary
                if variant == "plain":
                    level = noise_level_from_chunk_stats([float(np.sum(c)) for c in chunks], [float(np.max(c)) for c in chunks], chunk)
                    print(chunk, n_chunks, with_halo, "noise level", level)
                    assert (level > 0) == (n_chunks > 1)


def test_iir_cases_cover_the_sizes_and_values():
    cases = F.d_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    print(len(cases), "IIR cases")
    seen = set()
    for name, a, b, x in cases:
        assert a.dtype == b.dtype == np.float64 and x.dtype == np.complex64, name
        seen.add((len(a), len(b), len(x) - F.d_start(len(a), len(b))))
    for M, N in F.D_ORDERS:
        s = F.d_start(M, N)
        assert {(M, N, d) for d in (1 - s, -1, 0, 1, F.D_LONG - s)} <= seen, (M, N)
    by = dict((c[0], c) for c in cases)
    _, a, b, x = by["annexg_ff"]
    assert list(a) == [0.5] and len(b) == 0 and x[4] == complex(np.inf, np.inf) and x[8].real == -np.inf and x[8].imag == np.inf
    _, a, b, x = by["annexg_fb"]
    assert list(a) == [0.5, 0.25] and list(b) == [0.125] and x[4] == complex(np.inf, np.inf) and x[8].real == -np.inf
    _, a, b, x = by["grows_past_float32"]
    assert list(b) == [1.5] and len(x) == 400 and np.isfinite(x.view(np.float32)).all()
    # every special value is in some capture that is long enough to reach it, and every special coefficient in both places
    longs = np.concatenate([x for name, a, b, x in cases if name.endswith("_wild") and len(x) == F.D_LONG]).view(np.float32).reshape(-1, 2)
    for v in F.D_WILD:
        want = np.array([v.real, v.imag], np.float32).view(np.uint32)
        assert (longs.view(np.uint32) == want).all(axis=1).any(), v
    for tag in ("ap0", "an0", "ainf", "anan", "bp0", "bn0", "binf", "bnan"):
        assert any(n.endswith("_" + tag) for n in names), tag
    assert np.signbit(by["m3_n2_len4_an0"][1][0]) and np.isnan(by["m3_n2_len4_bnan"][2][-1])


# ---- the oracle against the recorded outputs of the reference ---------------------------------------------------------------------------
def test_golden_holds_the_cases_as_they_are_built(golden):
    """the recorded inputs are the builders' inputs bit for bit: the file and the GPU tests speak of the same cases"""
    assert os.path.getsize(F.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(F.GOLDEN), "fir_iir.npz"))
    built = {name: (x, h) for name, x, h in F.golden_fir_cases()}
    assert sorted(built) == sorted(golden["fir"]) and len(built) == 3
    for name, (x, h) in built.items():
        gx, gh, _ = golden["fir"][name]
        assert F.same_bits(gx, x) and F.same_bits(gh, h), name
    cases = F.d_cases()
    assert sorted(c[0] for c in cases) == sorted(golden["iir"])
    for name, a, b, x in cases:
        ga, gb, gx, gy = golden["iir"][name]
        assert np.array_equal(ga.view(np.uint64), a.view(np.uint64)) and np.array_equal(gb.view(np.uint64), b.view(np.uint64)), name
        assert F.same_bits(gx, x) and len(gy) == len(x), name
    assert sorted(golden["empty"]) == sorted(c[0] for c in F.e_cases())


def test_oracle_fir_equals_golden(oracle, golden):
    with np.errstate(all="ignore"):
        for name, (x, h, y) in golden["fir"].items():
            assert F.same_bits(oracle.fir_filter(x, h), y), name
    y = golden["fir"]["threshold_at"][2]
    assert np.isinf(y.real).any() and not np.isnan(y.view(np.float32)).any()


def test_oracle_iir_equals_golden(oracle, golden):
    with np.errstate(all="ignore"):
        for name, (a, b, x, y) in golden["iir"].items():
            assert F.same_bits(oracle.iir_filter(a, b, x), y), name
    # what the reference does with a sample of two infinite parts: it stays infinite (C99 Annex G), with and without feedback
    y = golden["iir"]["annexg_ff"][3]
    assert y[4] == complex(np.inf, np.inf) and y[8].real == -np.inf and y[8].imag == np.inf and np.isfinite(y[[3, 5, 7, 9]].view(np.float32)).all()
    y = golden["iir"]["annexg_fb"][3]
    assert (y[4:8] == complex(np.inf, np.inf)).all() and np.isnan(y[8].real) and y[8].imag == np.inf
    y = golden["iir"]["grows_past_float32"][3]
    assert np.isfinite(y[:150].view(np.float32)).all() and np.isinf(y[-1].real) and np.isinf(y[-1].imag)


def test_oracle_empty_taps_equal_golden(oracle, golden):
    """recorded from the reference: no taps give N - 1 zeros, no taps and no samples ValueError, no samples an empty array"""
    want = {"n5_m0": ("array", 4), "n0_m0": ("ValueError", None), "n0_m3": ("array", 0)}
    for name, (x, h, kind, y) in golden["empty"].items():
        assert (kind, None if y is None else len(y)) == want[name], name
        got_kind, got = F.fir_outcome(oracle.fir_filter, x, h)
        assert got_kind == kind, name
        if kind == "array":
            assert got.dtype == np.complex64 and F.same_bits(got, y) and not got.view(np.uint32).any(), name


# ---- the oracle against the reference itself, every family ------------------------------------------------------------------------------
def _fir_same(sf, oracle, x, h, what):
    with np.errstate(all="ignore"):
        assert F.same_bits(np.asarray(sf.fir_filter(x, h)), oracle.fir_filter(x, h)), what


def test_oracle_equals_reference_tap_counts(oracle):
    sf = _ref()
    for name, x, h in F.a_cases():
        _fir_same(sf, oracle, x, h, name)
    for name, x, h, cut in F.a_halo_cases():
        _fir_same(sf, oracle, x, h, name)
    for i, (x, h) in enumerate(F.a_sequence()):
        _fir_same(sf, oracle, x, h, i)


def test_oracle_equals_reference_checked_kernel_cases(oracle):
    sf = _ref()
    _fir_same(sf, oracle, *F.b_every_tile(), "every tile")
    halo, x, h = F.b_halo_tile0()
    _fir_same(sf, oracle, np.concatenate([halo, x]), h, "halo tile 0")
    for at in (False, True):
        _fir_same(sf, oracle, *F.b_threshold(at), at)


def test_oracle_equals_reference_statistics_cases(oracle):
    sf = _ref()
    import build_ref
    ref_util = build_ref.import_ref()[1]
    for chunk, n_chunks in F.C_GEOMETRIES:
        for with_halo in (False, True):
            for variant in F.C_VARIANTS:
                halo, x, h = F.c_case(chunk, n_chunks, variant, with_halo)
                full = x if halo is None else np.concatenate([halo, x])
                _fir_same(sf, oracle, full, h, (chunk, n_chunks, variant, with_halo))
                with np.errstate(all="ignore"):
                    iq = np.ascontiguousarray(oracle.fir_filter(full, h)).view(np.float32).reshape(-1, 2)
                    assert np.array_equal(np.asarray(ref_util.get_magnitudes(iq)), oracle.get_magnitudes(iq), equal_nan=True)


def test_oracle_equals_reference_iir_and_empty_taps(oracle):
    sf = _ref()
    with np.errstate(all="ignore"):
        for name, a, b, x in F.d_cases():
            assert F.same_bits(np.asarray(sf.iir_filter(a, b, x)), oracle.iir_filter(a, b, x)), name
    for name, x, h in F.e_cases():
        kind, want = F.fir_outcome(sf.fir_filter, x, h)
        got_kind, got = F.fir_outcome(oracle.fir_filter, x, h)
        assert got_kind == kind and (kind != "array" or (got.shape == want.shape and F.same_bits(got, want))), name
