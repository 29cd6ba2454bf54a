"""ShardedPipeline.iq_to_bits_auto on the CPU: the orchestration of urh_amd/sharding.py driven by the numpy model of the engine
(tests/model_shard_auto.py) over ThreadComm, against the oracle's chain on the whole capture:
detect_noise_level -> afp_demod -> detect_center -> grab_pulse_lens -> ppseq_to_bits_flat.  Every comparison is bit for bit."""
from dataclasses import replace

import numpy as np
import pytest

import center_cases as CC
import model_shard_auto as A
import model_shard_estimators as M
from urh_amd import sharding as S

N = 12_000


class CountingThreadComm(S.ThreadComm):
    """ThreadComm that counts the all-gathers a rank ENTERS"""

    def __init__(self, shared, rank):
        super().__init__(shared, rank)
        self.entered = 0

    def all_gather(self, t):
        self.entered += 1
        return super().all_gather(t)


def run_auto(oracle, iq, p, bounds, kw_for=None, engine_for=None, shard_for=None, timeout=120, runner=M.run_ranks, **kw):
    """iq_to_bits_auto on every rank -> (per rank: (piece, last_auto, last_center, engine, all-gathers entered), exceptions)"""
    n = len(iq)
    state = [None] * len(bounds)

    def work(r, comm):
        a, b = bounds[r]
        comm = CountingThreadComm(comm.shared, r)
        eng = engine_for(r) if engine_for else A.ModelAutoEngine(oracle.afp_demod)
        state[r] = (eng, comm)
        sp = S.ShardedPipeline(eng, comm)
        args = dict(kw)
        args.update(kw_for(r) if kw_for else {})
        res = sp.iq_to_bits_auto(shard_for(r) if shard_for else iq[a:b], p, pos_base=a, n_total=n, **args)
        return res, sp.last_auto, sp.last_center
    out, err = runner(len(bounds), work, timeout)
    return [None if o is None else o + (state[r][0], state[r][1].entered) for r, o in enumerate(out)], err, state


@pytest.fixture(scope="module")
def cases(oracle):
    """per (mod, dtype): the capture, parameters that are NOT the capture's, and the oracle's chain -- computed once, left unchanged"""
    cache = {}

    def get(mod, dtype):
        key = (mod, np.dtype(dtype).name)
        if key not in cache:
            iq = A.message_capture(N, mod, dtype, seed=len(cache) + 1)
            iq.setflags(write=False)
            p = A.params(mod)
            cache[key] = (iq, p, A.reference(oracle, iq, p), A.reference(oracle, iq, p, auto_noise=False, auto_center=False))
        return cache[key]
    return get


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.int8])
@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_auto_pass_equals_the_oracle_chain(oracle, cases, mod, dtype, world):
    iq, p, ref, plain = cases(mod, dtype)
    # the inputs make the test mean something
    assert ref["noise"] > 0
    assert ref["center"] is not None and ref["center"] != p.center
    assert not np.array_equal(ref["flat"][1], plain["flat"][1])
    assert len(ref["flat"][2]) > 3                                          # several messages
    out, err, _ = run_auto(oracle, iq, p, S.shard_bounds(N, world), auto_noise=True, auto_center=True)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), ref["flat"], (mod, dtype, world))
    qad = np.concatenate([o[0]["qad"] for o in out])
    assert np.array_equal(qad.view(np.uint32), ref["qad"].view(np.uint32))
    for _, auto, last_center, eng, _ in out:
        assert auto["noise"] == ref["noise"] and auto["center"] == ref["center"] == last_center and auto["center_detected"] is True
        assert eng.demod_calls == 1                                         # the shard is demodulated once


def test_seam_value_is_the_previous_sample_of_the_whole_capture(oracle, cases):
    """what the model's demod leaves: rows [a, b) of afp_demod(capture), and element a - 1 as the seam value"""
    for mod in ("ASK", "FSK"):
        iq, p, ref, _ = cases(mod, np.float32)
        p = replace(p, noise_threshold=ref["noise"])
        for r, (a, b) in enumerate(S.shard_bounds(N, 3)):
            eng = A.ModelAutoEngine(oracle.afp_demod)
            eng.demod(iq[a:b], None if r == 0 else iq[a - 2:a], a, N, r, 3, p)
            assert np.array_equal(eng.demod_qad().view(np.uint32), ref["qad"][a:b].view(np.uint32))
            assert r == 0 or np.float32(eng.demod_seam()).view(np.uint32) == ref["qad"][a - 1:a].view(np.uint32)[0]


@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_variants_equal_the_oracle_chain(oracle, cases, mod):
    """the halo handed over with the shard; auto_noise alone (the fused pass); auto_center alone"""
    iq, p, ref, _ = cases(mod, np.float32)
    bounds = S.shard_bounds(N, 3)
    out, err, _ = run_auto(oracle, iq, p, bounds, kw_for=lambda r: dict(left_halo=None if r == 0 else iq[bounds[r][0] - 2:bounds[r][0]]),
                           auto_noise=True, auto_center=True, halo_given=True)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), ref["flat"], "halo_given")
    want = A.reference(oracle, iq, p, auto_center=False)
    out, err, _ = run_auto(oracle, iq, p, bounds, auto_noise=True)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), want["flat"], "auto_noise alone")
    # noise + halo + summaries (+ merge) + flags
    assert all(o[1] == {"noise": want["noise"], "center": p.center, "center_detected": False, "all_gathers": 5 if mod == "ASK" else 4} for o in out)
    p2 = replace(p, noise_threshold=float(ref["noise"]) * 0.5)
    want = A.reference(oracle, iq, p2, auto_noise=False)
    out, err, _ = run_auto(oracle, iq, p2, bounds, auto_center=True)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), want["flat"], "auto_center alone")
    assert all(o[1]["noise"] is None and o[1]["center"] == want["center"] for o in out)


def test_center_not_found_uses_the_configured_center(oracle):
    """a constant-amplitude ASK capture: the demodulated signal has no variance, detect_center gives None on every rank"""
    iq = np.zeros((N, 2), np.float32)
    iq[:, 0] = 1.0
    p = A.params("ASK", center=0.5)
    ref = A.reference(oracle, iq, p, auto_noise=False)
    assert ref["center"] is None
    out, err, _ = run_auto(oracle, iq, p, S.shard_bounds(N, 3), auto_center=True)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), ref["flat"], "center None")
    for _, auto, last_center, _, _ in out:
        assert auto["center"] == p.center == last_center and auto["center_detected"] is False and auto["noise"] is None


def test_noise_level_not_below_max_magnitude_raises_on_every_rank(oracle):
    iq = A.loud_capture(6_400)
    noise = oracle.detect_noise_level(oracle.get_magnitudes(iq))
    assert noise >= 2 ** 0.5
    for kw in (dict(auto_noise=True, auto_center=True), dict(auto_noise=True)):
        out, err, state = run_auto(oracle, iq, A.params("FSK"), S.shard_bounds(len(iq), 3), timeout=30, runner=A.run_ranks_together, **kw)
        assert all(isinstance(e, ValueError) and "max_magnitude" in str(e) for e in err), err
        assert all(comm.entered == 1 and eng.demod_calls == 0 for eng, comm in state)      # the noise level's all-gather and no further one


REFUSALS = {
    "want_qad_false": (lambda r, iq, b: dict(want_qad=False) if r == 1 else {}, None, None, "want_qad"),
    "pipelined_engine": (None, lambda r, afp: A.ModelAutoEngine(afp, pipelined=(r == 1)), None, "pipelined"),
    "missing_left_halo": (lambda r, iq, b: dict(halo_given=True, left_halo=iq[b[r][0] - 2:b[r][0]] if r == 2 else None), None, None, "left_halo"),
    "non_contiguous_shard": (None, None, lambda r, iq, b: np.repeat(iq[b[r][0]:b[r][1]], 2, axis=0)[::2] if r == 1 else iq[b[r][0]:b[r][1]], "contiguous"),
}


@pytest.mark.parametrize("auto_noise", [False, True])
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_before_any_collective(oracle, cases, name, auto_noise):
    """rank 1 is wrong on its own: it raises ValueError before it enters a collective; the others are released (a broken barrier)"""
    iq, p, _, _ = cases("FSK", np.float32)
    bounds = S.shard_bounds(N, 3)
    kw_for, engine_for, shard_for, word = REFUSALS[name]
    out, err, state = run_auto(oracle, iq, p, bounds, kw_for=(lambda r: kw_for(r, iq, bounds)) if kw_for else None,
                               engine_for=(lambda r: engine_for(r, oracle.afp_demod)) if engine_for else None,
                               shard_for=(lambda r: shard_for(r, iq, bounds)) if shard_for else None, timeout=30,
                               auto_noise=auto_noise, auto_center=True)
    assert isinstance(err[1], ValueError) and word in str(err[1]), err
    assert state[1][1].entered == 0 and state[1][0].demod_calls == 0
    assert err[0] is not None and err[2] is not None and not isinstance(err[0], ValueError), err


def test_refusals_on_one_rank():
    sp = S.ShardedPipeline(A.ModelAutoEngine(None), S.ThreadComm(S.ThreadComm.Shared(1), 0))
    iq = np.zeros((100, 2), np.float32)
    with pytest.raises(ValueError, match="ASK, FSK and PSK"):
        sp.iq_to_bits_auto(iq, replace(A.params("FSK"), modulation_type="OQPSK"), auto_center=True)
    with pytest.raises(ValueError, match="inside the capture"):
        sp.iq_to_bits_auto(iq, A.params("FSK"), auto_center=True, pos_base=50, n_total=120)
    with pytest.raises(ValueError, match="two samples or fewer"):
        sp.iq_to_bits_auto(iq[:2], A.params("ASK"), auto_center=True)
    with pytest.raises(ValueError, match="max_size"):
        sp.iq_to_bits_auto(iq, A.params("ASK"), auto_center=True, center_max_size=-1)
    with pytest.raises(NotImplementedError, match="demod"):                  # an engine without the demodulation phase
        S.ShardedPipeline(M.ModelEstimatorEngine(), S.ThreadComm(S.ThreadComm.Shared(1), 0)).iq_to_bits_auto(iq, A.params("ASK"), auto_center=True)


@pytest.mark.parametrize("auto_noise", [False, True])
@pytest.mark.parametrize("halo_given", [False, True])
@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_collective_counts(oracle, cases, mod, halo_given, auto_noise):
    """the halo unless handed over, detect_center's four, summaries + (ASK) merge + flags, one more with auto_noise: no exchange of the
    shards' last demodulated values"""
    iq, p, ref, _ = cases(mod, np.float32)
    if not auto_noise:
        p = replace(p, noise_threshold=ref["noise"])
    bounds = S.shard_bounds(N, 3)
    y, _ = CC.histogram(ref["qad"], None)
    assert 1 < len(y) <= S.HIST_GATHER_BINS                               # detect_center: counts, two records, one block of the histogram
    out, err, _ = run_auto(oracle, iq, p, bounds, kw_for=lambda r: dict(left_halo=iq[bounds[r][0] - 2:bounds[r][0]] if (halo_given and r) else None),
                           auto_noise=auto_noise, auto_center=True, halo_given=halo_given)
    assert not any(err), err
    A.assert_flat_equal(S.stitch([o[0] for o in out]), ref["flat"], (mod, halo_given, auto_noise))
    want = (0 if halo_given else 1) + 4 + (3 if mod == "ASK" else 2) + (1 if auto_noise else 0)
    for _, auto, _, _, entered in out:
        assert auto["all_gathers"] == want == entered, (auto, entered, want)
