"""Pin the ORACLE on the batch's edge inputs (tests/batch_edge_cases.py) before the batch kernels are judged against it
(tests/test_batch_edges_gpu.py): against the real reference where oracle/_ref is built, and against the reference's committed outputs
(tests/golden/batch_edge/batch_edge.npz, tests/golden/make_batch_edge_golden.py) everywhere.  The builders' own conditions are asserted
here on the oracle's output, and printed, so that no case passes vacuously.  No GPU needed."""
import os

import numpy as np
import pytest

import batch_edge_cases as B
import edge_inputs as E
from conftest import ROOT

NAN_CAP = 0.02
MODS = ("FSK", "ASK")


@pytest.fixture(scope="module")
def S():
    from urh_amd.batch import batch_step
    return batch_step()


def _ref():
    import build_ref
    if not build_ref.built():
        pytest.skip("oracle/_ref not built (needs the reference)")
    return build_ref.import_ref()


def _assert_same_as_reference(sf, oracle, b, what=None):
    """afp_demod and grab_pulse_lens of the real reference against the oracle's on every capture of the batch"""
    with np.errstate(all="ignore"):
        for name, iq in b.caps:
            want = np.asarray(sf.afp_demod(iq, b.noise, b.mod, 2 ** b.bps))
            got, got_pp, _ = B.expected(oracle, iq, b)
            same = E.same_bits(want, got)
            assert want.shape == got.shape and same.all(), (b.tag, name, what, int((~same).sum()), np.nonzero(~same)[0][:5])
            pp = np.asarray(sf.grab_pulse_lens(want, b.center, b.tol, b.mod, b.sps, b.bps, b.spacing)).reshape(-1, 2)
            assert np.array_equal(pp, got_pp), (b.tag, name, what)


# ---- A1 --------------------------------------------------------------------------------------------------------------------------------------
def test_batch_positions_and_plans(S):
    n = B.n_small(S)
    clusters = B.batch_positions(n, S)
    last = (n - 1) // S * S
    assert clusters[:3] == [(0, 1, 2), (S - 1, S, S + 1), (2 * S - 1, 2 * S)] and clusters[-2:] == [(last - 1, last), (n - 1,)]
    inner = clusters[3:-2]
    assert len(inner) >= 6
    assert all(min(c) % S == 0 and max(c) % S == 1 or max(c) % S == S - 1 and min(c) % S == S - 2 for c in inner)
    assert any((min(c) // S) % 2 for c in inner) and any(not (min(c) // S) % 2 for c in inner)          # odd and even seams
    for c in inner:
        assert all(min(c) - max(o) >= 100 or min(o) - max(c) >= 100 for o in clusters if o is not c), c
    plans = B.batch_plans(n, S)
    assert sorted(plans) == list(E.VARIANTS)
    every = [x for v in plans for x in plans[v]]
    at63 = {name for pos, name, _ in every if pos % S == S - 1}
    at0 = {name for pos, name, _ in every if pos % S == 0}
    print("clusters", len(clusters), "specials at a lane 63:", len(at63), "at a lane 0:", len(at0), "of", len(E.SPECIALS))
    assert at63 == set(E.SPECIALS) and at0 == set(E.SPECIALS)
    assert {(name, mode) for _, name, mode in every} == {(name, m) for name in E.SPECIALS for m in (0, 1, 2)}
    hit = {pos for pos, _, _ in every}
    assert hit >= {0, 1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, last - 1, last, n - 1}
    for v in plans:                                        # one member of every cluster per capture
        assert len(plans[v]) == len(clusters) and len({p for p, _, _ in plans[v]}) == len(clusters)


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("mod", MODS)
def test_a1_nan_share(oracle, S, mod, bps):
    b = B.a1_batch(mod, bps, S)
    assert [n for n, _ in b.caps] == ["clean", "sprinkled0", "sprinkled1", "sprinkled2", "other", "clean"]
    for name, iq in b.caps[1:4]:
        qad = B.expected(oracle, iq, b)[0]
        share = float(np.isnan(qad).mean())
        print(b.tag, name, "NaN share %.4f" % share, "rows", len(B.expected(oracle, iq, b)[1]))
        assert 0 < share <= NAN_CAP
    qad, pp, flat = B.expected(oracle, b.caps[0][1], b)
    print(b.tag, "clean: rows", len(pp), "messages", len(flat[2]), "bits", len(flat[0]))
    assert not np.isnan(qad).any() and len(flat[2]) == 2 and len(pp) >= 20


@pytest.mark.parametrize("mod", MODS)
def test_a1_adjacent_captures_end_and_begin_non_finite(S, mod):
    b = B.a1_adjacent(mod, S)
    edge = b.arrays()[1:6]
    for a, c in zip(edge, edge[1:]):
        assert not np.isfinite(a[-1]).all() and not np.isfinite(c[0]).all()


# ---- A2 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mod", MODS)
def test_a2_scales_meet_their_conditions(oracle, S, mod):
    for k in B.SCALE_K:
        b = B.a2_batch(mod, 1, k, S)
        iq = b.caps[1][1]
        qad, pp, flat = B.expected(oracle, iq, b)
        with np.errstate(all="ignore"):
            m = iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]
        share = B.denormal_share(iq)
        print(b.tag, "denormal magnitudes %.3f" % share, "NOISE %.3f" % float((qad == oracle.noise_for_mod_type(mod)).mean()), "rows", len(pp),
              "bits", len(flat[0]))
        if k in B.DENORMAL_K:
            assert share > 0.5 and len(pp) >= 20
        if k == -76:
            assert (qad == oracle.noise_for_mod_type(mod)).all()
        if k == 64:
            assert np.isinf(m).any()


# ---- A3 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_a3_short_tie_captures_meet_the_long_ones_conditions(S, dtype):
    for b in B.a3_batch("FSK", dtype, 1, S):
        name, iq = b.caps[1]
        ties, above, below, split = B.tie_counts(iq, b.noise)
        print(b.tag, "samples", len(iq), "ties", ties, "above", above, "below", below, "runs of ties", len(E.tie_runs(iq, b.noise)),
              "float32 and exact arithmetic disagree on", split)
        assert (len(iq) - 9) % S == 0 and len(iq) >= 16 * S + 9
        assert ties >= 100 and above >= 100 and below >= 100 and len(E.tie_runs(iq, b.noise)) >= 10
        if name == "tie_full":
            assert split >= 20


def test_a3_tie_at_threshold_zero(oracle, S):
    for mod in MODS:
        b = B.a3_zero_threshold(mod, S)
        iq = b.caps[1][1]
        at = b.info["at"]
        assert (E.gate_classes(iq, 0.0) == 0).sum() == len(at) and S - 1 in at and S in at
        qad = B.expected(oracle, iq, b)[0]
        assert (qad[at] == oracle.noise_for_mod_type(mod)).all()


# ---- A4 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", B.INT_DTYPES)
def test_a4_range_grids_meet_their_conditions(oracle, S, dtype):
    v = B.range_values(dtype)
    info = np.iinfo(dtype)
    assert set(v) == {info.min, info.min + 1, (-1 if info.min < 0 else 1), 0, 1, info.max - 1, info.max}
    grid = B.range_grid(dtype, S)
    assert len(grid) == 20 * S + 9 and {(int(a), int(c)) for a, c in grid} == {(a, c) for a in v for c in v}
    assert (np.abs(np.diff(grid.astype(np.int64), axis=0)).sum(1) > 0).mean() > 0.9                        # neighbouring pairs vary
    for half in (False, True):
        b = B.a4_batch("ASK", dtype, half, S)
        qad = B.expected(oracle, b.caps[1][1], b)[0]
        ones = int((qad == np.float32(1.0)).sum())
        print(b.tag, "max %.5f" % float(qad.max()), "exactly 1.0:", ones, "above the center", int((qad > b.center).sum()), "NOISE",
              int((qad == 0).sum()))
        assert ones >= 28 and qad.max() > 1.0
        for mod in MODS:
            bb = B.a4_batch(mod, dtype, half, S)
            q = B.expected(oracle, bb.caps[1][1], bb)[0]
            live = q[q != oracle.noise_for_mod_type(mod)]
            assert (live > bb.center).sum() >= 20 and (live <= bb.center).sum() >= 20, (bb.tag, "one side of the center only")


# ---- A5 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_a5_samples_equal_the_threshold(oracle, S, dtype, bps):
    b = B.a5_batch(dtype, bps, S)
    iq = b.caps[1][1]
    qad, pp, _ = B.expected(oracle, iq, b)
    thr = oracle.get_center_thresholds(b.center, b.spacing, 2 ** bps)
    assert np.float32(b.center) == B.a5_threshold(dtype) and thr[2 ** bps // 2 - 1] == B.a5_threshold(dtype)
    equal = int((qad == B.a5_threshold(dtype)).sum())
    runs = E.longest_runs(qad == B.a5_threshold(dtype))
    below = B.a5_batch(dtype, bps, S, center=np.nextafter(B.a5_threshold(dtype), np.float32(-np.inf)))
    pp_below = B.expected(oracle, iq, below)[1]
    print(b.tag, "equal to the threshold", equal, "runs", len(runs), "rows", len(pp), "rows one float down", len(pp_below))
    assert equal >= 100 and (runs > b.tol).any() and (runs <= b.tol).any()
    assert (qad > B.a5_threshold(dtype)).sum() >= 100 and (qad < B.a5_threshold(dtype)).sum() >= 100
    assert not np.array_equal(pp, pp_below)                # `<=`: the equal value belongs to the state below


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------
def test_b1_first_state_is_that_of_zero(oracle):
    for tol in (0, 5):
        tables = {}
        for bps, spacing, center in B.B1_CASES:
            b = B.b1_batch(bps, spacing, center, tol)
            qad, pp, _ = B.expected(oracle, b.caps[0][1], b)
            assert len(b.caps[0][1]) == 1 and (qad == 0).all()
            tables[(bps, center)] = [B.expected(oracle, iq, b)[1].tolist() for _, iq in b.caps if len(iq) <= 2]
        print("tolerance", tol, {k: v[0] for k, v in tables.items()})
        states = {k: v[1][0][0] for k, v in tables.items()}            # (the capture of two samples)
        assert states[(1, -0.5)] != states[(1, 0.5)]
        assert len({states[(2, c)] for c in (-0.2, -0.05, 0.05, 0.2)}) == 4


@pytest.mark.parametrize("bps", [4, 5, 6, 7])
@pytest.mark.parametrize("mod", MODS)
def test_b2_many_states(oracle, S, mod, bps):
    b = B.b2_batch(mod, bps, S)
    iq = b.caps[0][1]
    qad, pp, flat = B.expected(oracle, iq, b)
    states = set(pp[:, 0].tolist()) - {-1}
    nsym = np.rint(pp[:, 1] / b.sps)
    pauses = nsym[pp[:, 0] == -1]
    print(b.tag, "samples", len(iq), "distinct states", len(states), "top", max(states), "rows", len(pp), "messages", len(flat[2]), "pauses", pauses)
    assert len(iq) == 30 * S + 9 and len(states) >= 2 ** bps // 2 and 2 ** bps - 1 in states
    assert (pauses > b.pt).any() and ((pauses > 0) & (pauses <= b.pt)).any()
    assert len(flat[2]) >= 2 and flat[0].any()


def test_b3_small_and_odd_samples_per_symbol(oracle):
    for sps in (1, 3, 7):
        b = B.b3_batch(sps)
        pp = B.expected(oracle, b.caps[0][1], b)[1]
        print(b.tag, "rows", len(pp))
        assert len(pp) >= 100 and b.tol == (0 if sps == 1 else 1) and b.pt == 8
        rr = np.abs(pp[:, 1]) % sps
        if sps > 1:
            assert (2 * rr > sps).any() and ((rr > 0) & (2 * rr < sps)).any()          # both sides of the rounding


@pytest.mark.parametrize("bps", [1, 3])
def test_b4_rows_of_more_than_64_symbols(oracle, bps):
    b = B.b4_batch(bps)
    pp, flat = B.expected(oracle, b.caps[0][1], b)[1:]
    nsym = np.floor(pp[:, 1] / b.sps + 0.5).astype(int).tolist()
    print(b.tag, "states", pp[:, 0].tolist(), "symbols", nsym)
    assert set(B.B4_SYMBOLS) <= set(nsym) and b.pt == 0
    assert pp[nsym.index(200), 0] == -1 and len(flat[0]) == sum(nsym) * bps
    assert set(pp[:, 0].tolist()) == {-1, 0, 2 ** bps - 1}


def test_c1_capture_has_50_to_200_rows(oracle):
    b = B.c1_batch()
    rows = [len(B.expected(oracle, iq, b)[1]) for iq in b.arrays()]
    print(b.tag, "rows", rows)
    assert rows[0] == 1 and rows[2] == 2 and 50 <= rows[1] <= 200


# ---- against the real reference ----------------------------------------------------------------------------------------------------------------
def _all_a_batches(S):
    out = []
    for mod in MODS:
        out += [B.a1_batch(mod, bps, S) for bps in (1, 2)] + [B.a1_adjacent(mod, S), B.a3_zero_threshold(mod, S)]
        out += [B.a2_batch(mod, bps, k, S) for bps in (1, 2) for k in B.SCALE_K]
        for dtype in E.DTYPES:
            for bps in ((1, 2) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.int16)) else (1,)):
                out += B.a3_batch(mod, dtype, bps, S)
        out += [B.a4_batch(mod, dtype, half, S) for dtype in B.INT_DTYPES for half in (False, True)]
    out += [B.a5_batch(dtype, bps, S) for dtype in (np.int8, np.float32) for bps in (1, 2)]
    return out


def test_oracle_equals_reference_on_the_value_cases(oracle, S):
    sf, _, _ = _ref()
    for b in _all_a_batches(S):
        _assert_same_as_reference(sf, oracle, b)


def test_oracle_equals_reference_on_the_parameter_cases(oracle, S):
    sf, _, _ = _ref()
    import ref_python
    ref_python.setup()
    from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer
    pa = ProtocolAnalyzer(None)
    batches = [B.b2_batch(mod, bps, S) for mod in MODS for bps in (4, 5, 6, 7)] + [B.b3_batch(sps) for sps in (1, 3, 7)]
    batches += [B.b4_batch(bps) for bps in (1, 3)] + [B.c1_batch()] + [B.b1_batch(bps, sp, c, tol) for bps, sp, c in B.B1_CASES for tol in (0, 5)]
    for b in batches:
        _assert_same_as_reference(sf, oracle, b)
        for name, iq in b.caps:
            _, pp, flat = B.expected(oracle, iq, b)
            ref = E.flatten_messages(*pa._ppseq_to_bits(pp, b.sps, b.bps, pause_threshold=b.pt))
            assert all(np.array_equal(x, y) for x, y in zip(ref, flat)), (b.tag, name)


# ---- against the reference's committed outputs ---------------------------------------------------------------------------------------------
def golden_cases(S):
    """[(name, batch, capture, stored with its input)]: the subset whose reference outputs are committed, one or more per group A1 .. A5"""
    out = []
    for mod in MODS:
        b = B.a1_batch(mod, 1, S)
        out.append(("A1/%s/sprinkled0" % mod, b, b.caps[1][1], False))
        for k in (-72, -64):
            b = B.a2_batch(mod, 1, k, S)
            out.append(("A2/%s/scaled%+d" % (mod, k), b, b.caps[1][1], False))
    for dtype in (np.int8, np.float32, np.int16):
        for b in B.a3_batch("FSK", dtype, 1, S):
            out.append((b.tag, b, b.caps[1][1], True))
    for mod, dtype in (("ASK", np.int8), ("ASK", np.uint16), ("FSK", np.int16)):
        b = B.a4_batch(mod, dtype, False, S)
        out.append((b.tag, b, b.caps[1][1], True))
    for dtype, bps in ((np.int8, 1), (np.float32, 2)):
        b = B.a5_batch(dtype, bps, S)
        out.append((b.tag, b, b.caps[1][1], True))
    return out


def test_oracle_equals_committed_reference_outputs(oracle, S):
    g = np.load(os.path.join(ROOT, "tests", "golden", "batch_edge", "batch_edge.npz"), allow_pickle=False)
    assert int(g["step"]) == S, "the fixture was recorded for another step: run tests/golden/make_batch_edge_golden.py where the reference is"
    cases = golden_cases(S)
    assert [str(n) for n in g["names"]] == [c[0] for c in cases]
    assert {c[0][:2] for c in cases} == {"A1", "A2", "A3", "A4", "A5"}
    for name, b, iq, with_input in cases:
        assert E.crc(iq) == int(g[name + "/crc"]), (name, "the builder no longer produces the capture the reference saw")
        assert float(g[name + "/noise"]) == b.noise and float(g[name + "/center"]) == b.center
        if with_input:
            assert np.array_equal(g[name + "/iq"], iq) and g[name + "/iq"].dtype == iq.dtype
        qad, pp, _ = B.expected(oracle, iq, b)
        same = E.same_bits(g[name + "/qad"], qad)
        assert same.all(), (name, int((~same).sum()), np.nonzero(~same)[0][:5])
        assert np.array_equal(g[name + "/pp"].reshape(-1, 2), pp), name
