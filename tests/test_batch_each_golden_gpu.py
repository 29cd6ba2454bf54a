"""A recording session end to end against the REAL reference (tests/golden/batch_each/batch_each.json, recorded by
tests/golden/make_batch_each_golden.py: Signal.auto_detect, then ProtocolAnalyzer.get_protocol_from_signal, per capture of every session of
tests/batch_estimate_cases.py): estimate_batch -> params_from_estimates -> get_protocols_from_signals_dev(captures, params), and
auto_detect_batch + get_protocols_batch on Signals, give the recorded messages -- bit string, pause, RSSI and timestamp by their bit
patterns, first position.  The recording asserts that the reference ends with PSK for no capture: no capture is left out but those for
which the reference raises, and those raise here too."""
import numpy as np
import pytest

import batch_each_cases as ec
import batch_estimate_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def gold():
    return ec.load()


def estimate_args(s):
    """what Signal.auto_detect hands AutoInterpretation.estimate for every capture of the session: its noise threshold, and "OOK" for ASK
    with one bit per symbol"""
    k = len(s["captures"])
    noise, mods = bc.per_capture(s["noise"], k), bc.per_capture(s["modulation"], k)
    return noise, [None if m is None else ("OOK" if m in ("ASK", "OOK") else m) for m in mods]


SESSIONS = sorted(bc.sessions())


def test_the_recording_covers_every_capture_and_holds_no_psk(gold):
    assert sorted(gold) == SESSIONS
    n_msg = 0
    for name, s in bc.sessions().items():
        assert len(gold[name]) == len(s["captures"])
        for e in gold[name]:
            if not isinstance(e, str):
                assert e["params"]["modulation_type"] in ("ASK", "FSK")
                n_msg += len(e["messages"])
    assert n_msg > 100 and len({(e["params"]["samples_per_symbol"], e["params"]["center"]) for es in gold.values() for e in es if not isinstance(e, str)}) > 20


@pytest.mark.parametrize("name", SESSIONS)
def test_estimate_then_protocols_with_a_parameter_set_per_capture(pipe, gold, name):
    from urh_amd.batch import params_from_estimates
    from urh_amd.protocol import get_protocols_from_signals_dev
    s, want = bc.sessions()[name], gold[name]
    caps = [np.ascontiguousarray(c) for c in s["captures"]]
    noise, mods = estimate_args(s)
    est = pipe.estimate_batch(caps, noise=noise, modulation=mods)
    keep, entries = [], []
    for k, w in enumerate(want):
        if isinstance(w, str):                                  # the reference raises for this capture: so does handing its estimate out
            with pytest.raises((ValueError, OverflowError)) as e:
                est[k]
            assert type(e.value).__name__ == w, (name, k)
            continue
        keep.append(k)
        entries.append(est[k])
    params = params_from_estimates(entries, [ec.demod_params(want[k]["base"]) for k in keep])
    for k, p, e in zip(keep, params, entries):
        r = want[k]["params"]
        assert (e is not None) == want[k]["detected"], (name, k)
        assert (p.modulation_type, p.bits_per_symbol, p.samples_per_symbol, p.tolerance, p.pause_threshold) == \
            (r["modulation_type"], r["bits_per_symbol"], r["samples_per_symbol"], r["tolerance"], r["pause_threshold"]), (name, k)
        assert p.center == r["center"] and np.float32(p.noise_threshold) == np.float32(r["noise_threshold"]), (name, k, p, r)
    got = get_protocols_from_signals_dev(pipe, [caps[k] for k in keep], params, 1, ec.SAMPLE_RATE, [ec.TIMESTAMP_STEP * k for k in keep])
    for k, msgs in zip(keep, got):
        ec.assert_messages(msgs, want[k]["messages"], (name, k))


def uniform(s):
    """(detect_modulation, detect_noise) where the session gives the modulation and the noise for all of its captures or for none, else None"""
    k = len(s["captures"])
    noise, mods = bc.per_capture(s["noise"], k), bc.per_capture(s["modulation"], k)
    if len({n is None for n in noise}) > 1 or len({m is None for m in mods}) > 1:
        return None
    return mods[0] is None, noise[0] is None


@pytest.mark.parametrize("name", [n for n in SESSIONS if uniform(bc.sessions()[n]) is not None])
def test_auto_detect_batch_then_get_protocols_batch(pipe, gold, name):
    from urh_amd.signal import Signal, auto_detect_batch, get_protocols_batch
    s, want = bc.sessions()[name], gold[name]
    keep = [k for k, w in enumerate(want) if not isinstance(w, str)]
    signals = []
    for k in keep:
        b = want[k]["base"]
        sig = Signal(np.ascontiguousarray(s["captures"][k]), modulation=b["modulation_type"], sample_rate=ec.SAMPLE_RATE, timestamp=ec.TIMESTAMP_STEP * k, pipe=pipe)
        for key in ("bits_per_symbol", "noise_threshold", "center", "center_spacing", "tolerance", "samples_per_symbol", "pause_threshold",
                    "message_length_divisor"):
            setattr(sig, key, b[key])
        signals.append(sig)
    found = auto_detect_batch(signals, *uniform(s))
    assert found == [want[k]["detected"] for k in keep]
    got = get_protocols_batch(signals)
    for k, sig, msgs in zip(keep, signals, got):
        assert sig.samples_per_symbol == want[k]["params"]["samples_per_symbol"] and sig.modulation_type == want[k]["params"]["modulation_type"], (name, k)
        ec.assert_messages(msgs, want[k]["messages"], (name, k))
