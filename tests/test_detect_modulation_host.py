"""What makes tests/test_detect_modulation_gpu.py trustworthy (no GPU): the cases of tests/modulation_cases.py and its float64
reference against the reference's own arithmetic.

Measured here (numpy 2.2, x86-64 longdouble), in the metric |delta var| / mean(m^2) of the magnitude array m:
  S = 6.91e-16   the largest difference between reference64 in float64 and in longdouble over families A-E (A_FSK_N32_len63)
  T = 256 S = 1.792e-13 from the recorded S = 7.0e-16: what the device's variances are held to (modulation_cases.T)
  the single-precision path (tests/numpy_estimators.py, the reference's arithmetic) lies up to 1.1e-7 from reference64, bound 1e-4
  the smallest relative margin of an inequality the reference evaluates is 1.15e-3 (A_PSK_N65536_len131071), bound 1e-3
Family F (8.4 million magnitudes) cannot keep every magnitude 1e-12 away from a float32 rounding boundary: 179 lie inside the
window, and rounded the other way they move the filtered variances by at most 2.8e-12 (first-order bound); its two filtered variances
are held to T plus that bound, everything else to T."""
import numpy as np
import pytest

import modulation_cases as M
import numpy_estimators

ALL = [n for f in M.FAMILIES for n in M.names(f)]
# the cases in which the reference returns before it computes a variance (8-bit noise is full of (0, 0) samples)
EARLY_EXITS = ["B_FSK_N16_s4_none", "B_FSK_N32_s8_none", "C_drop_4_exactly_ook", "G_int8_noise", "G_uint8_noise"]


def test_every_family_has_its_cases():
    for f in M.FAMILIES:
        assert len(M.names(f)) == M.COUNTS[f], (f, len(M.names(f)))
    assert len(ALL) == len(set(ALL)) == 184
    for n in ALL:
        c = M.case(n)
        assert c.msg.dtype == np.complex64 and not c.msg.flags.writeable and 1 <= c.order <= 16 and c.scale >= 1, n
    assert set(M.E_EXPECT) == set(M.names("E")) and set(M.G_RAW) == set(M.names("G"))
    # the shapes the families are there for
    assert {M.ref(n).info["N"] for n in M.names("A")} == set(M.A_SIZES)
    assert sorted(M.ref(n).info["n_dropped"] for n in M.names("C"))[-2:] == [3, 4]
    f = M.case("F_FSK_1026_tiles")
    assert len(f.msg) == 1026 * 4096 + 7 and M.ref(f.name).info["N"] == 2 ** 22 and M.ref(f.name).info["n_dropped"] == 2
    assert M.ref("C_len_N_plus_2_three_zeros_halves").info["N"] == 2048 and M.ref("C_len_N_plus_2_three_zeros_ask").info["N"] == 128


def test_same_labels_as_the_single_precision_path_and_the_reference():
    ref_dm = None
    import build_ref
    import ref_python
    if build_ref.built() and ref_python.available():
        ref_python.setup()
        from urh.ainterpretation import AutoInterpretation as AI
        ref_dm = AI.detect_modulation
    seen = set()
    for n in ALL:
        c, r = M.case(n), M.ref(n)
        with np.errstate(all="ignore"):
            assert r.label == numpy_estimators.detect_modulation(c.msg.copy(), c.scale, c.order), n
            if ref_dm is not None:
                assert r.label == ref_dm(c.msg.copy(), c.scale, c.order), n
        seen.add(r.label)
    assert seen == {"FSK", "ASK", "PSK", "OOK", None}
    for n, want in M.E_EXPECT.items():                      # family E: the label each message was built for, decided in the last branch
        assert M.ref(n).label == want and M.ref(n).info["top"] is not None, (n, M.ref(n).label, M.ref(n).info["top"])
    # the early exits return before any variance; every other case has four numbers, NaN only in the two variances whose
    # unit-magnitude input overflowed (1 / 1e-42 in float32)
    for n in ALL:
        r = M.ref(n)
        if r.info["mags"] is None:
            assert np.isnan(r.variances).all() and r.label in (None, "OOK"), n
        elif n == "C_denormal_1e-42":
            assert np.isnan(r.variances).tolist() == [False, True, False, True], r.variances
        else:
            assert np.isfinite(r.variances).all(), (n, r.variances)
    assert [n for n in ALL if M.ref(n).info["mags"] is None] == EARLY_EXITS


def test_every_inequality_has_its_margin():
    worst = min(ALL, key=lambda n: M.min_margin(M.ref(n)))
    print("smallest margin %.3g in %s" % (M.min_margin(M.ref(worst)), worst))
    for n in ALL:
        for text, lhs, rhs, margin in M.ref(n).info["margins"]:
            assert margin >= M.MARGIN, (n, text, lhs, rhs, margin)
    for n in M.names("E"):                                  # the magnitude limit: below 90 or above 110 against 100
        mags = [lhs for text, lhs, rhs, margin in M.ref(n).info["margins"] if text.startswith("fft[")]
        assert all(v < 90 or v > 110 for v in mags), (n, mags)
    assert M.ref("E_N256_mag_below_90_ook").info["top"][1][1] < 90 and M.ref("E_N2048_mag_below_90_ook").info["top"][1][1] < 90
    # distances 9 and 10 exactly
    for n in M.names("E"):
        top = M.ref(n).info["top"]
        d = abs(top[1][0] - top[0][0])
        assert d == (9 if "dist9" in n else 10 if "dist10" in n else d) and d >= 9, (n, top[:2])
    N = 2048
    per = -(-N // 64)
    same, other = M.ref("E_N2048_dist10_fsk_one_slice").info["top"], M.ref("E_N2048_dist10_fsk_two_slices").info["top"]
    assert same[0][0] // per == same[1][0] // per and other[0][0] // per != other[1][0] // per
    assert M.ref("E_N2048_second_peak_at_slice_end_fsk").info["top"][1][0] % per == per - 1
    assert M.ref("E_N2048_peak_at_shifted_0_fsk").info["top"][0][0] == 0 and M.ref("E_N2048_second_peak_at_shifted_0_fsk").info["top"][1][0] == 0
    assert M.ref("E_N2048_peak_at_shifted_last_fsk").info["top"][0][0] == N - 1
    assert M.ref("E_N2048_second_peak_at_shifted_last_fsk").info["top"][1][0] == N - 1


def test_no_magnitude_on_a_float32_rounding_boundary():
    strict = 0
    for n in ALL:
        r = M.ref(n)
        if r.info["mags"] is None:
            continue
        h1, h2, e2, e3 = M.boundary_exposure(r, M.case(n).order)
        if r.info["N"] <= M.STRICT_BOUNDARY_MAX_N:
            assert h1 == 0 and h2 == 0, (n, h1, h2)
            assert (M.tolerance(n) == M.T).all()
            strict += 1
        else:
            print("%s: %d + %d magnitudes in the window, filtered variances exposed by %.3g, %.3g" % (n, h1, h2, e2, e3))
            assert n == "F_FSK_1026_tiles" and 0 < max(e2, e3) < 4e-12
            assert (M.tolerance(n) <= 1e-11).all() and (M.tolerance(n)[:2] == M.T).all()
    assert strict == len(ALL) - len(EARLY_EXITS) - 1


def test_the_measured_spread():
    s, worst = 0.0, None
    for f in "ABCDE":
        for n in M.names(f):
            a, b = M.ref(n), M.ref(n, True)
            assert a.label == b.label, n
            if a.info["mags"] is None:
                continue
            assert b.info["mags"][0].dtype == np.longdouble
            m = float(M.metric(a.variances, b.variances, a).max())
            if m > s:
                s, worst = m, n
    print("S = %.3g (%s), recorded S = %.3g, T = 256 S = %.4g" % (s, worst, M.S, M.T))
    assert np.finfo(np.longdouble).eps < 2e-19             # an 80-bit longdouble, or S measures nothing
    assert 0 < s <= M.S and M.T == 256 * M.S and M.T <= 1e-11


def test_the_single_precision_path_stays_near_the_float64_reference():
    worst = 0.0
    for f in "ABCDEG":
        for n in M.names(f):
            r = M.ref(n)
            if r.info["mags"] is None:
                continue
            m = M.metric(M.single_precision_variances(M.case(n)), r.variances, r)
            worst = max(worst, float(m.max()))
            assert (m <= 1e-4).all(), (n, m)
    print("single precision against float64: %.3g" % worst)


def test_boundary_hits_finds_a_midpoint():
    a = np.float32(1.2345678)
    b = np.nextafter(a, np.float32(2))
    mid = 0.5 * (float(a) + float(b))
    got = M.boundary_hits(np.array([float(a), mid, mid * (1 + 5e-13), mid * (1 - 5e-13), mid * (1 + 4e-12), float(b), np.nan]))
    assert got.tolist() == [1, 2, 3]
