"""Pin the ORACLE on the edge-value inputs (tests/edge_inputs.py) before the kernels are judged against it
(tests/test_edge_values.py): against the real reference where oracle/_ref is built, and against the reference's committed outputs
(tests/golden/edge/edge.npz, tests/golden/make_edge_golden.py) everywhere.  The builders' own conditions -- NaN share, ties on the
gate, share of products inside the division's window, NaN runs and threshold-equal samples in the pulse-table input -- are asserted
here on the oracle's output, so that no case passes vacuously."""
import os

import numpy as np
import pytest

import edge_inputs as E
from conftest import ROOT

MODS = ("FSK", "ASK", "PSK")
NAN_CAP = {"FSK": 0.02, "ASK": 0.02, "PSK": 0.15}


def _ref():
    import build_ref
    if not build_ref.built():
        pytest.skip("oracle/_ref not built (needs the reference)")
    return build_ref.import_ref()


def _assert_demod_equal(a, b, mod, what):
    st = 1 if mod == "PSK" else 0                          # the reference leaves result[0] of PSK unwritten
    same = E.same_bits(a[st:], b[st:])
    assert a.shape == b.shape and same.all(), (what, int((~same).sum()), np.nonzero(~same)[0][:5] + st)


# ---- the builders' conditions (no reference needed) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("mod", MODS)
def test_float_cases_meet_their_conditions(oracle, mod, order):
    with np.errstate(all="ignore"):
        for dev in ((20e3, 140e3) if mod == "FSK" else (20e3,)):
            cases = E.float_cases(mod, order, dev)
            assert len(cases) == len(E.VARIANTS) + len(E.SCALE_K) + (mod == "PSK")
            for tag, iq, noise, _, _ in cases:
                qad = oracle.afp_demod(iq, noise, mod, order)[1:]
                share = float(np.isnan(qad).mean())
                print(mod, order, int(dev), tag, "NaN share %.4f" % share, "inside the window %.3f" % E.inside_window_share(iq))
                assert share <= NAN_CAP[mod], (mod, order, tag, share)
                if tag.startswith("sprinkled") or tag == "nan_in_gap":
                    assert share > 0                       # the specials did reach the output
                if tag in ("scaled-20", "scaled+20") and mod != "ASK":      # (the ASK pass forms no conjugate product)
                    assert 0.05 <= E.inside_window_share(iq) <= 0.95, (mod, tag)
                if tag == "scaled-76":
                    assert (iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1] == 0).any()
                    assert (qad == oracle.noise_for_mod_type(mod)).all()    # 0 <= 0: NOISE
                if tag == "scaled+64":
                    assert np.isinf(iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]).any()


def test_sprinkle_plans_cover_every_special_and_position():
    for psk, n in ((False, E.N_DEFAULT), (True, E.N_PSK)):
        plans = [E.sprinkle_plan(n, v, psk) for v in E.VARIANTS]
        for plan in plans:
            pos = [p for p, _, _ in plan]
            assert all(b - a >= 300 for a, b in zip(pos, pos[1:]))
            assert {name for _, name, _ in plan} == set(E.SPECIALS)
        if not psk:                                                 # every special in every component, over the variants
            assert {(name, mode) for plan in plans for _, name, mode in plan} == {(name, m) for name in E.SPECIALS for m in (0, 1, 2)}
        hit = {p for plan in plans for p, _, _ in plan}
        assert hit >= {0, 1, 2, n - 1, 2047, 2048, 8191, 8192, 8193}
        assert any(p % 128 == 0 for p in hit) and any(p % 128 == 127 for p in hit) and any(p % 128 == 1 for p in hit) and any(p % 128 == 126 for p in hit)
        if psk:
            assert hit >= {4095, 4096, 4097, 3 * 4096 + 1 - 200}
            for plan in plans:                                      # NaN / inf in the last tenth only
                assert all((name in E.NONFINITE) == (p >= n - n // 10) for p, name, _ in plan)


def test_psk_nan_in_gap_poisons_from_its_sample_on(oracle):
    for order in (2, 4):
        iq, noise, pos = E.psk_nan_in_gap(order)
        clean = iq.copy()
        clean[pos, 0] = 0.0
        assert (E.gate_classes(clean[pos - 200:pos + 200], noise) <= 0).all()          # the NaN sits inside a gated stretch
        with np.errstate(all="ignore"):
            qad = oracle.afp_demod(iq, noise, "PSK", order)
        assert not np.isnan(qad[1:pos]).any() and np.isnan(qad[pos])                    # not gated: NaN <= x is false
        assert (qad[pos + 1:pos + 200] == -4.0).all()                                   # the gated samples after it still are
        later = qad[pos + 300:]
        assert np.isnan(later[later != -4.0]).all() and np.isnan(later).sum() > 1000     # ... and the loop stays poisoned


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_tie_captures_meet_their_conditions(dtype):
    for tag, iq, nt, _, _ in E.tie_cases("FSK", dtype):
        g = E.gate_classes(iq, nt)
        ties, above, below = int((g == 0).sum()), int((g > 0).sum()), int((g < 0).sum())
        print(np.dtype(dtype).name, tag, "ties", ties, "above", above, "below", below, "runs of ties", len(E.tie_runs(iq, nt)))
        assert ties >= 100 and above >= 100 and below >= 100
        assert len(E.tie_runs(iq, nt)) >= 10
        if tag == "tie_full":
            split = int(((g > 0) != (E.exact_gate_classes(iq, nt) > 0)).sum())
            print("float32 and exact arithmetic disagree on", split)
            assert split >= 20


def test_tie_at_threshold_zero(oracle):
    """noise_threshold = 0: a sample whose squares underflow to zero is a tie (0 <= 0: NOISE)"""
    iq, _ = E.base_capture("FSK")
    iq = E.sprinkle(iq, [500, 900], [(E.SPECIALS["+1e-30"], E.SPECIALS["-1e-30"]), (E.SPECIALS["+1e-40"], E.SPECIALS["-0"])])
    assert (E.gate_classes(iq, 0.0) == 0).sum() == 2
    for mod in MODS:
        qad = oracle.afp_demod(iq, 0.0, mod, 2)
        assert qad[500] == oracle.noise_for_mod_type(mod) and qad[900] == oracle.noise_for_mod_type(mod)


@pytest.mark.parametrize("mod", MODS)
def test_rect_with_specials_meets_its_conditions(oracle, mod):
    for order in (2, 4):
        x, center, spacing = E.rect_with_specials(order, mod)
        th = oracle.get_center_thresholds(center, spacing, order)
        assert np.array_equal(th, E.center_thresholds(center, spacing, order))
        runs = E.longest_runs(np.isnan(x))
        assert int(np.isin(x, th).sum()) >= 20
        for tol in (2, 3, 5):
            assert (runs > tol).any() and (runs <= tol).any()
        assert np.isposinf(x).any() and np.isneginf(x).any()
        noise_val = np.float32(oracle.noise_for_mod_type(mod))
        assert (x == np.nextafter(noise_val, np.float32(np.inf))).any() and (x == np.nextafter(noise_val, np.float32(-np.inf))).any()
        # a NaN lands in the TOP state: a NaN run longer than the tolerance gives a row of state order - 1 where the level below it is 0
        pp = oracle.grab_pulse_lens(np.where(np.isnan(x), np.float32(np.nan), np.float32(th[0] - 1)), center, 2, "FSK", 40, order.bit_length() - 1, spacing)
        assert int((pp[:, 0] == order - 1).sum()) == int((runs > 2).sum()) > 0 and -1 not in pp[:, 0]


# ---- against the real reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("mod", MODS)
def test_oracle_demod_equals_reference_on_float_edge_values(oracle, mod, order):
    sf, _, _ = _ref()
    with np.errstate(all="ignore"):
        for dev in ((20e3, 140e3) if mod == "FSK" else (20e3,)):
            for tag, iq, noise, _, _ in E.float_cases(mod, order, dev):
                _assert_demod_equal(np.asarray(sf.afp_demod(iq, noise, mod, order)), oracle.afp_demod(iq, noise, mod, order), mod, (mod, order, dev, tag))
        for bw in (0.05,) if mod == "PSK" else ():
            for tag, iq, noise, _, _ in E.float_cases(mod, order, variants=(0,), ks=(-20, 64)):
                _assert_demod_equal(np.asarray(sf.afp_demod(iq, noise, mod, order, bw)), oracle.afp_demod(iq, noise, mod, order, bw), mod, (mod, order, bw, tag))


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_oracle_demod_equals_reference_on_ties(oracle, dtype):
    sf, _, _ = _ref()
    for mod in MODS:
        for order in (2, 4):
            for tag, iq, nt, _, _ in E.tie_cases(mod, dtype, order):
                _assert_demod_equal(np.asarray(sf.afp_demod(iq, nt, mod, order)), oracle.afp_demod(iq, nt, mod, order), mod, (mod, order, tag))


def test_oracle_pulse_table_equals_reference_on_specials(oracle):
    sf, _, _ = _ref()
    import ref_python
    ref_python.setup()
    from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer
    pa = ProtocolAnalyzer(None)
    for mod in MODS:
        for order in (2, 4):
            x, center, spacing = E.rect_with_specials(order, mod)
            for tol in (0, 1, 5):
                for bps in (1, 2):
                    want = np.asarray(sf.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing))
                    got = oracle.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing)
                    assert np.array_equal(want, got), (mod, order, tol, bps)
                    ref = E.flatten_messages(*pa._ppseq_to_bits(want, 40, bps, pause_threshold=8))
                    flat = oracle.ppseq_to_bits_flat(got, 40, bps, True, 8)
                    assert all(np.array_equal(a, b) for a, b in zip(ref, flat)), (mod, order, tol, bps)


# ---- against the reference's committed outputs -----------------------------------------------------------------------------------------
def test_oracle_equals_committed_reference_outputs(oracle):
    g = np.load(os.path.join(ROOT, "tests", "golden", "edge", "edge.npz"), allow_pickle=False)
    names = [str(n) for n in g["names"]]
    demod, rect = E.golden_demod_cases(), E.golden_rect_cases()
    assert names == [c[0] for c in demod] + [c[0] for c in rect] and len(names) == 25
    with np.errstate(all="ignore"):
        for name, mod, order, iq, noise, with_input in demod:
            assert E.crc(iq) == int(g[name + "/crc"]), (name, "the builder no longer produces the capture the reference saw")
            assert float(g[name + "/noise"]) == noise
            if with_input:
                assert np.array_equal(g[name + "/iq"], iq)
            _assert_demod_equal(g[name + "/qad"], oracle.afp_demod(iq, noise, mod, order), mod, name)
    for name, mod, bps, x, center, spacing, tol in rect:
        assert np.array_equal(g[name + "/x"].view(np.uint32), x.view(np.uint32)), name
        pp = oracle.grab_pulse_lens(x, center, tol, mod, 40, bps, spacing)
        assert np.array_equal(pp, g[name + "/pp"]), name
        flat = oracle.ppseq_to_bits_flat(pp, 40, bps, True, 8)
        for key, a in zip(("bits", "msg_off", "pauses", "pos", "pos_off"), flat):
            assert np.array_equal(a, g[name + "/" + key]), (name, key)
