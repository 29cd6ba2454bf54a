"""The scenarios of tests/estimate_route_cases.py are what they claim, told from the recorded reference results
(tests/golden/estimate_routes.json) and from the captures themselves; where the real reference is built, the record is what the recorder
writes today, and the oracle's restatement agrees with it on the parts it covers.  No GPU needed."""
import numpy as np
import pytest

import estimate_route_cases as rc

POOL_BINS, MSG_GROUP, TIE_BATCH, WINDOW = 4096, 4096, 1024, 1 << 16


def test_every_scenario_is_recorded_and_answers_with_a_dict():
    rec = rc.load_record()
    assert sorted(rec) == sorted(rc.scenarios())
    for name, s in rc.scenarios().items():
        assert len(rec[name]) == len(s["captures"]), name
        for i, c in enumerate(rec[name]):
            if c["estimate"] is None:                    # only the noise-only and the empty capture of the session
                assert name.startswith("session-pooled") and i in (17, 30) and c["messages"] == 0, (name, i)
            else:
                assert set(c["estimate"]) == {"modulation_type", "bit_length", "center", "tolerance", "noise"} and c["messages"] > 0, (name, i)
                assert c["estimate"]["modulation_type"] != "PSK", (name, i)
    routes = set(r for s in rc.scenarios().values() for r in s["routes"])
    assert routes == {f"R{k}" for k in range(1, 10)}


def test_the_recorded_counts_exceed_the_capacities_they_are_meant_to():
    from urh_amd import batch, estimators
    assert (estimators.CAP_SEG, estimators.CAP_MERGED, estimators._TIE_BATCH, batch.MSG_GROUP) == (4096, 65536, TIE_BATCH, MSG_GROUP)
    rec = rc.load_record()
    for name, n in (("many-fsk-4200", 4200), ("many-fsk-8300", 8300), ("many-fsk-cut-4096", 4096), ("many-fsk-cut-4097", 4097)):
        assert rec[name][0]["segments"] == rec[name][0]["messages"] == n, name
        assert rec[name][0]["estimate"]["bit_length"] == rc.MANY_SPS and rec[name][0]["estimate"]["tolerance"] == 1
    assert 8300 > 2 * POOL_BINS and 8300 % POOL_BINS                      # three batches of center statistics, the last one partial
    for name in ("long-lead", "long-lead-retry"):
        assert rec[name][0]["outlasting"] == 1 and rec[name][0]["messages"] <= POOL_BINS
    assert rec["long-lead"][0]["estimate"]["bit_length"] == 100 and rec["long-lead"][0]["plateaus"] < WINDOW < rec["long-lead-retry"][0]["plateaus"]
    assert len(rc.scenarios()["long-lead-retry"]["captures"][0]) < 4_000_000
    assert rec["flat-tone"][0]["bins_over_pool"] == 1 and rec["flat-tone"][0]["messages"] == 5
    for mod in ("FSK", "ASK"):
        assert rec[f"tied-peaks-{mod}"][0]["tied"] >= 1 and rec[f"tied-peaks-{mod}"][0]["bins_over_pool"] == 0
        assert rec[f"equal-counts-{mod}"][0]["equal_counts"] >= 1 and rec[f"equal-counts-{mod}"][0]["tied"] == 0
    assert rec["tied-many"][0]["tied"] == rc.TIED_MANY > TIE_BATCH
    ook = rec["ook-bursts"][0]
    assert ook["segments"] > ook["messages"] > rc.OOK_MERGED_CAP and ook["messages"] >= rc.OOK_BURSTS


def test_the_pooled_boundary_falls_inside_a_capture():
    """the FSK captures' messages, pooled in the order given, are cut at batch.MSG_GROUP: not between two captures; the captures' lengths are
    mixed so that the longest-first launch order is not the order given"""
    for name in ("session-pooled", "session-pooled-detect"):
        rec = rc.load_record()[name]
        counts = [c["messages"] for c in rec if c["modulation"] == "FSK"]
        ends = np.cumsum(counts)
        assert ends[-1] > MSG_GROUP and MSG_GROUP not in ends.tolist(), name
        inside = int(np.searchsorted(ends, MSG_GROUP))
        assert ends[inside] - counts[inside] < MSG_GROUP < ends[inside] and inside < len(counts) - 1
        assert 0 < sum(c["messages"] for c in rec if c["modulation"] in ("OOK", "ASK")) <= MSG_GROUP
    caps = rc.scenarios()["session-pooled"]["captures"]
    lengths = [len(c) for c in caps]
    assert len(caps) == 45 and lengths[30] == 0 and lengths != sorted(lengths, reverse=True) and len(set(lengths)) > 30
    assert sum(lengths) < 4_000_000 and max(lengths) < 196_608            # (every capture stays inside the batch)
    assert rc.scenarios()["session-pooled-detect"]["modulation"] is None
    # the vote names the modulation each capture was made with
    made = rc.scenarios()["session-pooled"]["modulation"]
    seen = [c["modulation"] for c in rc.load_record()["session-pooled-detect"]]
    assert all(s == m for s, m, c in zip(seen, made, rc.load_record()["session-pooled-detect"]) if c["messages"])


def test_the_integer_captures_use_their_full_range():
    for dt in (np.uint8, np.uint16, np.int8, np.int16):
        info = np.iinfo(dt)
        s = rc.scenarios()[f"unsigned-{np.dtype(dt).name}"]
        assert s["modulation"] == ["FSK", "ASK"]
        fsk, ask = s["captures"]
        assert fsk.dtype == ask.dtype == np.dtype(dt)
        span = float(info.max) - float(info.min)
        assert float(fsk.max()) - float(fsk.min()) > 0.9 * span
        assert float(ask.max()) > info.max - 0.15 * span
        if np.dtype(dt).kind == "u":                                      # the floor sits in the middle of the range, not at 0
            assert abs(float(np.median(fsk)) - (info.max + 1) / 2) < 0.02 * span
    assert len(rc.scenarios()["many-fsk-4200"]["captures"][0]) == 4200 * rc.MANY_STRIDE + rc.MANY_GAP
    assert max(len(c) for s in rc.scenarios().values() for c in s["captures"]) < 12_000_000


def test_vote_on_messages_gives_the_recorded_estimate(oracle):
    """estimators.vote_on_messages on per-message values computed WITHOUT the library's device code (the oracle and tests/numpy_estimators.py),
    for the scenarios small enough for the oracle's loops"""
    import numpy_estimators as np_est
    from test_batch_estimate_host import _per_message_values
    from urh_amd.estimators import vote_on_messages
    import model_batch_segments as model
    for name in ("tied-peaks-FSK", "tied-peaks-ASK", "equal-counts-FSK", "equal-counts-ASK"):
        s = rc.scenarios()[name]
        want = rc.expected(name)[0]
        iq = np.array(s["captures"][0])
        segments = oracle.segment_messages_from_magnitudes(model.magnitudes(iq), want["noise"])
        assert len(segments) == rc.load_record()[name][0]["segments"], name
        assert [list(x) for x in (segments[:1] + segments[-1:])] == rc.load_record()[name][0]["ranges"], name
        cen, tol, bl = _per_message_values(np_est, oracle, iq, want["noise"], s["modulation"], segments)
        got = vote_on_messages(s["modulation"], want["noise"], cen, tol, bl)
        assert rc.same_estimate(got, want), (name, got, want)


def test_the_record_is_what_the_reference_says_today():
    """where the real reference is built: the recorder's figures for the scenarios that take it a moment, equal to the committed record"""
    import ref_python
    if not ref_python.available():
        pytest.skip("the reference is not built here")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_estimate_routes_golden", os.path.join(rc.ROOT, "tests", "golden", "make_estimate_routes_golden.py"))
    rec_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec_mod)
    for name in ("long-lead", "flat-tone", "tied-peaks-FSK", "equal-counts-ASK", "unsigned-uint8", "unsigned-uint16"):
        s = rc.scenarios()[name]
        k = len(s["captures"])
        for i, (iq, nz, m) in enumerate(zip(s["captures"], rc.per_capture(s["noise"], k), rc.per_capture(s["modulation"], k))):
            r = rec_mod.plain(rec_mod.AI.estimate(np.array(iq), noise=nz, modulation=m))
            want = rc.load_record()[name][i]
            assert r == want["estimate"], (name, i, r)
            a = rec_mod.anatomy(iq, r["noise"], m)
            assert {key: want[key] for key in a} == a, (name, i, a)
