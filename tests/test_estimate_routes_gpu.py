"""Every route around the fast path of estimators.estimate_dev and DevicePipeline.estimate_batch, end to end against the recorded answers of
the real reference (tests/estimate_route_cases.py, tests/golden/estimate_routes.json), with no tolerance anywhere -- and, from the trace of the
native calls, the proof that the route each scenario exists for was taken."""
import numpy as np
import pytest

import estimate_route_cases as rc
from call_trace import recording

pytestmark = pytest.mark.gpu

# plain integer arguments: capacities and message counts
INT_ARGS = {"urhgpu_message_ranges_dev": (6, 9), "urhgpu_message_ranges_demod_dev": (6, 9), "urhgpu_msg_estimate": (4,), "urhgpu_msg_center_stats": (4,),
            "urhgpu_msg_plateau_decisions": (5,), "urhgpu_msg_plateaus": (5, 10), "urhgpu_msg_bit_lengths": (2,)}


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def _dev(pipe, a):
    return pipe.torch.from_numpy(np.array(a)).to(pipe.device)              # (a copy: the cases are read-only)


def _options(name):
    s = rc.scenarios()[name]
    k = len(s["captures"])
    return s, rc.per_capture(s["noise"], k), rc.per_capture(s["modulation"], k)


def _alone(pipe, name, i=0):
    from urh_amd.estimators import estimate_dev
    s, noise, mods = _options(name)
    return estimate_dev(pipe, _dev(pipe, s["captures"][i]), noise=noise[i], modulation=mods[i])


def _traced(fn):
    with recording(INT_ARGS) as rec:
        got = fn()
    return got, list(rec.log)


def _positions(log, *wanted):
    """the positions of `wanted` in the trace, each looked for behind the one before it: a call is matched by its whole line, or by its name
    where no argument is given"""
    at, out = 0, []
    for w in wanted:
        hits = [i for i in range(at, len(log)) if log[i] == w or (" " not in w and log[i].split()[0] == w)]
        assert hits, (w, "not in the trace behind position", at, [c for c in log if c.split()[0] == w.split()[0]][:8])
        out.append(hits[0])
        at = hits[0] + 1
    return out


def _count(log, name):
    return sum(1 for c in log if c.split()[0] == name)


def _check(name, got, i=0):
    want = rc.expected(name)[i]
    assert rc.same_estimate(got, want), (name, i, got, want)


# ---- every scenario: estimate_dev and estimate_batch against the record ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.scenarios()))
def test_estimate_dev_and_estimate_batch_equal_the_reference(pipe, name):
    """estimate_dev of capture k == the reference's AutoInterpretation.estimate (recorded) == entry k of estimate_batch over the scenario"""
    s, noise, mods = _options(name)
    want = rc.expected(name)
    assert len(want) == len(s["captures"])
    alone = [_alone(pipe, name, i) for i in range(len(want))]
    for i, (a, w) in enumerate(zip(alone, want)):
        assert rc.same_estimate(a, w), (name, i, a, w)
    got = pipe.estimate_batch(s["captures"], noise=s["noise"], modulation=s["modulation"])
    assert len(got) == len(want)
    for i in range(len(want)):
        assert rc.same_estimate(got[i], want[i]), (name, i, got[i], want[i])
        assert rc.same_estimate(got[i], alone[i]), (name, i, got[i], alone[i])


# ---- R1, R4: more segments than the first call holds, more messages than urhgpu_msg_estimate takes ---------------------------------------
@pytest.mark.parametrize("name", ["many-fsk-4200", "many-fsk-8300", "many-fsk-cut-4097"])
def test_more_than_4096_messages_take_the_second_ranges_call_and_the_two_stage_decisions(pipe, name):
    from urh_amd import estimators
    n = rc.load_record()[name][0]["segments"]
    assert n > estimators.CAP_SEG and n == rc.load_record()[name][0]["messages"]
    got, log = _traced(lambda: _alone(pipe, name))
    _check(name, got)
    _positions(log, f"urhgpu_message_ranges_dev {estimators.CAP_SEG} {estimators.CAP_MERGED}", f"urhgpu_message_ranges_dev {n} 0",                     # R1
               f"urhgpu_msg_estimate {n}", f"urhgpu_msg_center_stats {n}", f"urhgpu_msg_plateau_decisions {n}")                                       # R4
    assert _count(log, "urhgpu_message_ranges_dev") == 2 and _count(log, "urhgpu_msg_estimate") == 1
    assert _count(log, "urhgpu_bit_length_from_order") > 0               # (a quarter of these short messages have equal counts: R8 on the way)


def test_exactly_4096_messages_stay_on_the_fast_path(pipe):
    from urh_amd import estimators
    name = "many-fsk-cut-4096"
    assert rc.load_record()[name][0]["segments"] == estimators.CAP_SEG == 4096
    got, log = _traced(lambda: _alone(pipe, name))
    _check(name, got)
    assert _count(log, "urhgpu_message_ranges_dev") == 1 and _count(log, "urhgpu_msg_estimate") == 1
    assert f"urhgpu_msg_center_stats {4096}" not in log and f"urhgpu_msg_plateau_decisions {4096}" not in log


def test_one_call_and_two_calls_decide_the_same_messages_alike(pipe):
    """message_decisions on the first 4096 messages (one urhgpu_msg_estimate) and on 4097 (refused: center statistics, then the plateau
    decisions): the same three arrays for the messages they share"""
    from urh_amd import estimators
    from urh_amd.pipeline import DemodParams
    iq = _dev(pipe, rc.scenarios()["many-fsk-cut-4097"]["captures"][0])
    ranges = estimators.message_ranges_dev(pipe, iq, 0.1, merge=False, cap_seg=5000)[0]
    assert len(ranges) == 4097
    data = pipe.afp_demod(iq, DemodParams("FSK", 1, 0.1))
    one, log1 = _traced(lambda: estimators.message_decisions(pipe, data, ranges[:4096]))
    two, log2 = _traced(lambda: estimators.message_decisions(pipe, data, ranges))
    assert "urhgpu_msg_center_stats 4096" not in log1 and "urhgpu_msg_plateau_decisions 4096" not in log1
    _positions(log2, "urhgpu_msg_estimate 4097", "urhgpu_msg_center_stats 4097", "urhgpu_msg_plateau_decisions 4097")
    for a, b in zip(one, two):
        assert a.dtype == b.dtype and np.array_equal(a, b[:4096], equal_nan=a.dtype.kind == "f")
    assert (one[0] == one[0]).any() and (one[2] > 0).any()                          # (centers and bit lengths, not a row of "none")


# ---- R2, R3: the OOK merge ----------------------------------------------------------------------------------------------------------------
def test_more_merged_bursts_than_the_capacity_take_the_second_ranges_call(pipe, monkeypatch):
    from urh_amd import estimators
    c = rc.load_record()["ook-bursts"][0]
    assert c["messages"] > rc.OOK_MERGED_CAP and c["segments"] <= estimators.CAP_SEG
    monkeypatch.setattr(estimators, "CAP_MERGED", rc.OOK_MERGED_CAP)
    got, log = _traced(lambda: _alone(pipe, "ook-bursts"))
    _check("ook-bursts", got)
    _positions(log, f"urhgpu_message_ranges_demod_dev {estimators.CAP_SEG} {rc.OOK_MERGED_CAP}", f"urhgpu_message_ranges_dev 1 {c['messages']}",
               f"urhgpu_msg_estimate {c['messages']}")
    assert _count(log, "urhgpu_segment_runs_dev") == 0


def test_an_ambiguous_merge_is_decided_by_numpy_as_the_reference_decides_it(pipe):
    from urh_amd import _lib
    c = rc.load_record()["ook-bursts"][0]
    lib = _lib.load()
    lib.urhgpu_test_force_merge_ambiguous(1)
    try:
        got, log = _traced(lambda: _alone(pipe, "ook-bursts"))
    finally:
        lib.urhgpu_test_force_merge_ambiguous(0)
    _check("ook-bursts", got)
    _positions(log, "urhgpu_message_ranges_demod_dev", "urhgpu_segment_runs_dev", f"urhgpu_msg_estimate {c['messages']}")
    assert _count(log, "urhgpu_message_ranges_dev") == 0


# ---- R5, R6: centers the device cannot settle --------------------------------------------------------------------------------------------
def test_a_message_with_more_bins_than_the_pool_takes_the_single_message_center(pipe):
    c = rc.load_record()["flat-tone"][0]
    assert c["bins_over_pool"] == 1 and c["tied"] == 0
    got, log = _traced(lambda: _alone(pipe, "flat-tone"))
    _check("flat-tone", got)
    _positions(log, f"urhgpu_msg_estimate {c['messages']}", "urhgpu_compact_gt_dev", "urhgpu_histogram_f32_dev", "urhgpu_msg_plateau_decisions 1")
    assert _count(log, "urhgpu_histogram_f32_dev") == 1


@pytest.mark.parametrize("name", ["tied-peaks-FSK", "tied-peaks-ASK", "tied-many"])
def test_tied_peaks_are_decided_by_numpy_on_the_fetched_histograms(pipe, name):
    from urh_amd import estimators
    c = rc.load_record()[name][0]
    ties = c["tied"]
    assert ties > (estimators._TIE_BATCH if name == "tied-many" else 0) and c["bins_over_pool"] == 0
    got, log = _traced(lambda: _alone(pipe, name))
    _check(name, got)
    batches = [min(estimators._TIE_BATCH, ties - a) for a in range(0, ties, estimators._TIE_BATCH)]
    _positions(log, f"urhgpu_msg_estimate {c['messages']}", *[f"urhgpu_msg_center_stats {b}" for b in batches], f"urhgpu_msg_plateau_decisions {ties}")
    assert _count(log, "urhgpu_msg_center_stats") == len(batches) and _count(log, "urhgpu_histogram_f32_dev") == 0


# ---- R7, R8: plateau decisions the device hands back -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,calls", [("long-lead", 1), ("long-lead-retry", 2)])
def test_a_first_plateau_beyond_the_window_sends_all_messages_through_the_sequence_path(pipe, name, calls):
    c = rc.load_record()[name][0]
    n = c["messages"]
    assert c["outlasting"] == 1 and n <= 4096 and (c["plateaus"] > (1 << 16)) == (calls == 2)
    got, log = _traced(lambda: _alone(pipe, name))
    _check(name, got)
    assert got["bit_length"] == (100 if name == "long-lead" else 8)
    first = _positions(log, f"urhgpu_msg_estimate {n}", f"urhgpu_msg_plateaus {n} {1 << 16}")[1]
    _positions(log[first:], "urhgpu_msg_plateaus", "urhgpu_edges_le_dev", f"urhgpu_msg_bit_lengths {n}")
    assert _count(log, "urhgpu_msg_plateaus") == calls
    if calls == 2:                                           # the retry asks for what the first call counted: more than it had room for
        again = [x for x in log if x.split()[0] == "urhgpu_msg_plateaus"][1].split()
        assert int(again[1]) == n and int(again[2]) > (1 << 16)


@pytest.mark.parametrize("name", ["equal-counts-FSK", "equal-counts-ASK"])
def test_equal_counts_in_the_divisor_histogram_are_ordered_by_numpy(pipe, name):
    c = rc.load_record()[name][0]
    assert c["equal_counts"] > 0 and c["tied"] == 0 and c["outlasting"] == 0 and c["bins_over_pool"] == 0
    got, log = _traced(lambda: _alone(pipe, name))
    _check(name, got)
    _positions(log, f"urhgpu_msg_estimate {c['messages']}", "urhgpu_edges_le_dev", "urhgpu_msg_divisor_histogram", "urhgpu_bit_length_from_order")
    assert _count(log, "urhgpu_msg_plateaus") == 0 and _count(log, "urhgpu_msg_center_stats") == 0


# ---- R9: a session with more pooled messages than one group ------------------------------------------------------------------------------
def _group(name, *mods):
    return sum(c["messages"] for c in rc.load_record()[name] if c["modulation"] in mods)


@pytest.mark.parametrize("name", ["session-pooled", "session-pooled-detect"])
def test_a_session_of_more_than_one_group_is_decided_in_chunks(pipe, name):
    """list and packed device input; the FSK captures' messages are more than batch.MSG_GROUP: two urhgpu_msg_estimate rounds for that group, one
    for the ASK captures in front of them, none for a capture alone"""
    from urh_amd import batch
    s = rc.scenarios()[name]
    want = rc.expected(name)
    total, ask = _group(name, "FSK"), _group(name, "OOK", "ASK")
    assert total > batch.MSG_GROUP == 4096 and 0 < ask <= 4096
    caps = s["captures"]
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    for form, given in (("list", caps), ("packed", (_dev(pipe, np.concatenate(caps)), starts))):
        got, log = _traced(lambda: list(pipe.estimate_batch(given, noise=s["noise"], modulation=s["modulation"])))
        assert len(got) == len(want)
        for i in range(len(want)):
            assert rc.same_estimate(got[i], want[i]), (name, form, i, got[i], want[i])
        assert [x for x in log if x.split()[0] == "urhgpu_msg_estimate"] == [f"urhgpu_msg_estimate {ask}", "urhgpu_msg_estimate 4096",
                                                                              f"urhgpu_msg_estimate {total - 4096}"], form
        assert _count(log, "urhgpu_message_ranges_dev") == 0 and _count(log, "urhgpu_message_ranges_demod_dev") == 0       # (no capture went alone)
    assert want[17] is None and want[30] is None and sum(w is None for w in want) == 2


def test_one_capture_of_more_messages_than_a_group_as_a_batch_of_one(pipe):
    """the 4200-message capture kept inside the batch (long_from above its length): its messages are pooled and cut at batch.MSG_GROUP"""
    name = "many-fsk-4200"
    s = rc.scenarios()[name]
    n = rc.load_record()[name][0]["messages"]
    got, log = _traced(lambda: list(pipe.estimate_batch(s["captures"], noise=s["noise"], modulation=s["modulation"], long_from=2 ** 31 - 1)))
    assert len(got) == 1
    _check(name, got[0])
    assert [x for x in log if x.split()[0] == "urhgpu_msg_estimate"] == ["urhgpu_msg_estimate 4096", f"urhgpu_msg_estimate {n - 4096}"]
    assert _count(log, "urhgpu_message_ranges_dev") == 0 and _count(log, "urhgpu_msg_center_stats") <= 2      # (at most a tie per chunk)


# ---- what the estimate is handed to --------------------------------------------------------------------------------------------------------
def _applied(sig):
    return (sig.modulation_type, int(sig.samples_per_symbol), int(sig.tolerance), float(sig.center), float(sig.noise_threshold))


def _as_applied(est):
    return (est["modulation_type"], est["bit_length"], est["tolerance"], est["center"], est["noise"])


def test_auto_detect_sets_what_the_record_says(pipe):
    from urh_amd.signal import Signal, auto_detect_batch
    s = rc.scenarios()["many-fsk-4200"]
    sig = Signal(s["captures"][0], pipe=pipe, modulation="FSK")
    sig.noise_threshold = s["noise"]
    assert sig.auto_detect(detect_modulation=False, detect_noise=False) is True
    assert _applied(sig) == _as_applied(rc.expected("many-fsk-4200")[0])
    name = "session-pooled-detect"
    s, want = rc.scenarios()[name], rc.expected(name)
    keep = [i for i, c in enumerate(s["captures"]) if len(c)]
    assert sum(rc.load_record()[name][i]["messages"] for i in keep if rc.load_record()[name][i]["modulation"] == "FSK") > 4096
    sigs = [Signal(s["captures"][i], pipe=pipe) for i in keep]
    for x in sigs:
        x.noise_threshold = s["noise"]
    ret = auto_detect_batch(sigs, detect_modulation=True, detect_noise=False)
    assert ret == [want[i] is not None for i in keep] and ret.count(False) == 1
    for x, i in zip(sigs, keep):
        if want[i] is not None:
            assert _applied(x) == _as_applied(want[i]), i
