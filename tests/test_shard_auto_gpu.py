"""ShardedPipeline.iq_to_bits_auto on the GPU: W ranks as threads on the one GPU, one GpuShardEngine each, ThreadComm.  The demodulation
phase alone (urhgpu_shard_demod_dev: k_afp_demod and the streaming kernel's demodulation-only instantiation with a real halo, the seam
value) against the oracle's afp_demod of the whole capture; the whole pass against the oracle's chain
(detect_noise_level -> afp_demod -> detect_center -> grab_pulse_lens -> ppseq_to_bits_flat) AND the single-GPU pass
DevicePipeline.iq_to_bits(auto_noise=True, auto_center=True).  Every comparison is bit for bit."""
from dataclasses import replace

import numpy as np
import pytest

import model_shard_auto as A
import model_shard_estimators as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def engines():
    from urh_amd.shard_engine import GpuShardEngine
    return [GpuShardEngine(0) for _ in range(8)]


def to_dev(iq):
    import torch
    a = np.ascontiguousarray(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. the demodulation phase alone -------------------------------------------------------------------------------------------------
def gate(dtype):
    """a noise threshold that gates the gaps of message_capture (unsigned samples, which are not centred: about half of all samples)"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return 0.25
    info = np.iinfo(dtype)
    if dtype.kind == "u":
        return 0.5 * min(info.max, 32767) * 2 ** 0.5
    return 0.1 * info.max


def bounds_of(n, world):
    from urh_amd.sharding import shard_bounds
    return shard_bounds(n, world)


GEOMETRIES = {
    # every shard below 8192 samples: only k_afp_demod runs, with a real halo
    "n6400_w2": (6_400, 2), "n6400_w3": (6_400, 3),
    # shards of exactly 4, 2 and 1 chunks of 8192: only the streaming instantiation runs, with a real halo
    "n65536_w2": (65_536, 2), "n65536_w4": (65_536, 4), "n65536_w8": (65_536, 8),
    # whole chunks plus a remainder (its halo lies inside the shard), the last shard of odd length
    "n100003_w3": (100_003, 3), "n300007_w8": (300_007, 8),
    # a 64-sample shard between two others
    "explicit": (20_000, [(0, 8_192), (8_192, 8_256), (8_256, 20_000)]),
}


def geometry(name):
    n, w = GEOMETRIES[name]
    return n, (w if isinstance(w, list) else bounds_of(n, w))


def test_geometries_are_what_their_names_say():
    for name, want in (("n6400_w2", lambda s: max(s) < 8192), ("n6400_w3", lambda s: max(s) < 8192),
                       ("n65536_w2", lambda s: set(s) == {4 * 8192}), ("n65536_w4", lambda s: set(s) == {2 * 8192}), ("n65536_w8", lambda s: set(s) == {8192}),
                       ("n100003_w3", lambda s: all(v > 8192 and v % 8192 for v in s) and s[-1] % 2 == 1),
                       ("n300007_w8", lambda s: all(v > 8192 and v % 8192 for v in s) and s[-1] % 2 == 1), ("explicit", lambda s: s[1] == 64)):
        n, bounds = geometry(name)
        assert bounds[0][0] == 0 and bounds[-1][1] == n and all(bounds[r][1] == bounds[r + 1][0] for r in range(len(bounds) - 1))
        assert want([b - a for a, b in bounds]), (name, bounds)


@pytest.fixture(scope="module")
def demod_inputs(oracle):
    """per (mod, dtype, n): the capture on the GPU, the parameters and the oracle's afp_demod of the whole capture -- computed once"""
    cache = {}

    def get(mod, dtype, n, **kw):
        key = (mod, np.dtype(dtype).name, n, tuple(sorted(kw.items())))
        if key not in cache:
            iq = A.message_capture(n, mod, dtype, seed=n % 97 + np.dtype(dtype).itemsize, **kw)
            p = replace(A.params(mod), noise_threshold=gate(dtype))
            want = oracle.afp_demod(iq, p.noise_threshold, mod, 2)
            want.setflags(write=False)
            cache[key] = (to_dev(iq), p, want)
        return cache[key]
    return get


def demodulate_shards(engines, dev, bounds, p):
    """the demodulation phase of every rank, one after the other -> per rank (qad on the host, seam value or None)"""
    n, out = int(dev.shape[0]), []
    for r, (a, b) in enumerate(bounds):
        e = engines[r]
        left = None if r == 0 else dev[a - 2:a]
        e.demod_own(dev[a:b], left)
        e.demod(dev[a:b], left, a, n, r, len(bounds), p)
        out.append((e.demod_qad().cpu().numpy().copy(), e.demod_seam() if r > 0 else None))
        e._pre = None                                     # the pass ends here: nothing runs behind the demodulation
    return out


def assert_demodulated(got, bounds, want, what):
    for r, ((qad, seam), (a, b)) in enumerate(zip(got, bounds)):
        bad = np.nonzero(bits32(qad) != bits32(want[a:b]))[0]
        assert qad.shape == (b - a,) and len(bad) == 0, (what, r, (a, b), len(bad), bad[:8], qad[bad[:8]], want[a:b][bad[:8]])
        if r > 0:
            assert bits32(seam) == bits32(want[a - 1:a])[0], (what, r, a, seam, want[a - 1])


@pytest.mark.parametrize("geom", sorted(GEOMETRIES))
@pytest.mark.parametrize("dtype", A.SAMPLE_TYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_demodulation_phase_equals_oracle_rows(engines, demod_inputs, mod, dtype, geom):
    n, bounds = geometry(geom)
    dev, p, want = demod_inputs(mod, dtype, n)
    noise_val = np.float32(0.0 if mod == "ASK" else -4.0)
    gated = int((want == noise_val).sum())
    assert want[0] == noise_val and 0 < gated < n                       # the gate takes some samples and leaves some
    assert_demodulated(demodulate_shards(engines, dev, bounds, p), bounds, want, (mod, dtype, geom))


@pytest.mark.parametrize("mod", ["ASK", "FSK"])
def test_seam_value_below_and_above_the_gate(engines, demod_inputs, mod):
    """the sample before the second seam is exactly zero (below the gate): its seam value is the NOISE constant; the one before the first
    seam lies in a burst: a real value"""
    n, bounds = geometry("explicit")
    dev, p, want = demod_inputs(mod, np.float32, n, blank=(8_255, 8_256))
    noise_val = np.float32(0.0 if mod == "ASK" else -4.0)
    assert want[8_191] != noise_val and want[8_255] == noise_val and want[8_254] != noise_val and want[8_256] != noise_val
    got = demodulate_shards(engines, dev, bounds, p)
    assert_demodulated(got, bounds, want, (mod, "seam"))
    assert got[1][1] != noise_val and got[2][1] == noise_val


def test_demodulation_phase_refuses_what_it_does_not_do(engines, demod_inputs):
    from urh_amd import _lib
    n, bounds = geometry("n6400_w2")
    dev, p, _ = demod_inputs("FSK", np.float32, n)
    e = engines[0]
    with pytest.raises(_lib.UrhGpuError):                                 # PSK has its Costas phases
        e.demod(dev[:3200], None, 0, n, 0, 2, replace(p, modulation_type="PSK"))
    with pytest.raises(_lib.UrhGpuError):                                 # rank 1 without its halo
        e.demod(dev[3200:], None, 3200, n, 1, 2, p)
    e._pre = None


# ---- 2. the whole pass ------------------------------------------------------------------------------------------------------------------
N_PASS = 100_003
KINDS = {"ASK": ("ASK", 2), "FSK2": ("FSK", 2), "FSK4": ("FSK", 4)}
ASK_LOW, ASK_BLANK = (33_200, 33_500), (33_300, 33_312)       # around the first seam of three ranks (33 344), inside a burst


def single_flat(res):
    return (res.ppseq().copy(),) + tuple(x.copy() for x in res.flat())


@pytest.fixture(scope="module")
def pass_inputs(pipe, oracle):
    """per (kind, dtype): capture, parameters that are NOT the capture's, the oracle's chain and the single-GPU pass -- computed once"""
    cache = {}

    def get(kind, dtype):
        key = (kind, np.dtype(dtype).name)
        if key not in cache:
            mod, order = KINDS[kind]
            extra = dict(low=ASK_LOW, blank=ASK_BLANK) if mod == "ASK" else {}
            iq = A.message_capture(N_PASS, mod, dtype, seed=7 + order, order=order, **extra)
            p = A.params(mod, order)
            dev = to_dev(iq)
            ref = A.reference(oracle, iq, p)
            plain = A.reference(oracle, iq, p, auto_noise=False, auto_center=False)
            # the inputs make the test mean something
            assert ref["noise"] > 0 and ref["center"] is not None and ref["center"] != p.center
            assert not np.array_equal(ref["flat"][1], plain["flat"][1]) and len(ref["flat"][2]) > 3
            res = pipe.iq_to_bits(dev, p, want_qad=True, auto_noise=True, auto_center=True)
            single = dict(flat=single_flat(res), noise=res.noise_threshold, center=res.center)
            cache[key] = (iq, dev, p, ref, single)
        return cache[key]
    return get


def run_auto(engines, dev, bounds, p, kw_for=None, shard_for=None, timeout=120, runner=M.run_ranks, **kw):
    """iq_to_bits_auto on every rank -> (per rank dict(piece, qad, auto, center, absorbed, res), exceptions)"""
    from urh_amd import _lib
    from urh_amd.sharding import ShardedPipeline
    n = int(dev.shape[0])

    def work(r, comm):
        sp = ShardedPipeline(engines[r], comm)
        a, b = bounds[r]
        args = dict(kw)
        args.update(kw_for(r) if kw_for else {})
        res = sp.iq_to_bits_auto(shard_for(r) if shard_for else dev[a:b], p, pos_base=a, n_total=n, **args)
        piece = res.piece()                                # (the engine's buffers are reused by its next pass)
        absorbed = res.host_counts()[0] > 0 and int(res.rows_buf[0, 0].item()) == _lib.ROW_ABSORBED
        return dict(piece=piece, qad=res.qad.cpu().numpy().copy() if res.qad is not None else None, auto=sp.last_auto, center=sp.last_center,
                    absorbed=absorbed, res=res)
    return runner(len(bounds), work, timeout)


def stitched(out):
    from urh_amd.sharding import stitch
    return stitch([o["piece"] for o in out])


def seams_inside_runs(ppseq, bounds):
    """the seams that lie strictly inside a row of the pulse table (a run of equal states)"""
    ends = set(np.cumsum(ppseq[:, 1]).tolist())
    return [a for a, _ in bounds[1:] if a not in ends]


@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_auto_pass_equals_oracle_and_single_gpu(engines, pass_inputs, kind, dtype, world):
    iq, dev, p, ref, single = pass_inputs(kind, dtype)
    bounds = bounds_of(N_PASS, world)
    assert len(seams_inside_runs(ref["flat"][0], bounds)) >= 1             # a seam inside a run of equal states
    out, err = run_auto(engines, dev, bounds, p, auto_noise=True, auto_center=True)
    assert not any(err), err
    what = (kind, dtype, world)
    A.assert_flat_equal(stitched(out), ref["flat"], what + ("oracle",))
    A.assert_flat_equal(stitched(out), single["flat"], what + ("single GPU",))
    qad = np.concatenate([o["qad"] for o in out])
    assert np.array_equal(bits32(qad), bits32(ref["qad"])), what
    gathers = 1 + 1 + 4 + (3 if kind == "ASK" else 2)                      # noise, halo, detect_center, summaries (+ merge) + flags
    for o in out:
        assert o["auto"] == {"noise": ref["noise"], "center": ref["center"], "center_detected": True, "all_gathers": gathers}, (what, o["auto"])
        assert o["center"] == ref["center"] == single["center"] and o["auto"]["noise"] == single["noise"], what
    if kind == "ASK" and dtype == np.float32 and world == 3:
        # rank 0's last row and the row that spans the first seam have the same state: the merge exchange gives rank 1's first row to rank 0
        assert out[1]["absorbed"] and not out[0]["absorbed"], [o["absorbed"] for o in out]


@pytest.mark.parametrize("kind", ["ASK", "FSK2"])
def test_variants_equal_the_single_gpu_pass(pipe, engines, pass_inputs, kind):
    """the halo handed over with the shard; auto_noise alone (the fused pass); auto_center alone"""
    iq, dev, p, ref, single = pass_inputs(kind, np.float32)
    bounds = bounds_of(N_PASS, 3)
    halos = [None] + [dev[a - 2:a].clone() for a, _ in bounds[1:]]
    out, err = run_auto(engines, dev, bounds, p, kw_for=lambda r: dict(left_halo=halos[r]), auto_noise=True, auto_center=True, halo_given=True)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), single["flat"], (kind, "halo_given"))
    assert all(o["auto"]["all_gathers"] == 1 + 4 + (3 if kind == "ASK" else 2) for o in out)
    want = pipe.iq_to_bits(dev, p, want_qad=True, auto_noise=True)
    want_flat, want_noise = single_flat(want), want.noise_threshold
    out, err = run_auto(engines, dev, bounds, p, auto_noise=True)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), want_flat, (kind, "auto_noise alone"))
    assert all(o["auto"] == {"noise": want_noise, "center": p.center, "center_detected": False, "all_gathers": 5 if kind == "ASK" else 4} for o in out)
    p2 = replace(p, noise_threshold=float(ref["noise"]) * 0.5)
    want = pipe.iq_to_bits(dev, p2, want_qad=True, auto_center=True)
    want_flat, want_center = single_flat(want), want.center
    assert want_center is not None
    out, err = run_auto(engines, dev, bounds, p2, auto_center=True)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), want_flat, (kind, "auto_center alone"))
    assert all(o["auto"]["noise"] is None and o["center"] == want_center for o in out)


def test_a_fused_pass_after_the_demodulation_phase_is_the_fused_pass(engines, pass_inputs):
    """a demodulation phase that no runs phase followed does not change what iq_to_bits does on the same engine and the same buffers"""
    from urh_amd.sharding import ShardedPipeline
    iq, dev, p, ref, single = pass_inputs("FSK2", np.float32)
    p = replace(p, noise_threshold=ref["noise"], center=ref["center"])
    bounds = bounds_of(N_PASS, 2)
    demodulate_shards(engines, dev, bounds, replace(p, noise_threshold=0.0))       # another gate: the qad it leaves is not this pass's

    def work(r, comm):
        a, b = bounds[r]
        res = ShardedPipeline(engines[r], comm).iq_to_bits(dev[a:b], p, pos_base=a, n_total=N_PASS)
        return dict(piece=res.piece(), qad=res.qad.cpu().numpy().copy())
    out, err = M.run_ranks(2, work)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), ref["flat"], "fused")
    assert np.array_equal(bits32(np.concatenate([o["qad"] for o in out])), bits32(ref["qad"]))


# ---- 3. dc_correct -> the automatic pass -> message_records ----------------------------------------------------------------------------
def test_corrected_automatic_pass_with_records(pipe, engines):
    import msg_record_cases as mc
    import shard_record_cases as sc
    from urh_amd import sharding as S
    n, world, divisor = N_PASS, 3, 8
    iq = A.message_capture(n, "ASK", np.int16, seed=21, low=ASK_LOW, blank=None, offset=0.05)
    p, dev = A.params("ASK"), to_dev(iq)
    whole = pipe.iq_to_bits(dev, p, want_qad=True, dc_correction=True, auto_noise=True, auto_center=True, msg_records=True, message_length_divisor=divisor)
    want_rec, want_msgs, want_flat = whole.records.copy(), whole.message_data(), single_flat(whole)
    assert len(want_rec) > 3 and whole.center is not None and whole.noise_threshold > 0
    bounds = bounds_of(n, world)

    def work(r, comm):
        sp = S.ShardedPipeline(engines[r], comm)
        a, b = bounds[r]
        shard, halo = dev[a:b].clone(), None
        if r > 0:
            shard, (halo,) = sp.dc_correct(shard, pos_base=a, n_total=n, also=[dev[a - 2:a].clone()])
        else:
            shard = sp.dc_correct(shard, pos_base=a, n_total=n)
        res = sp.iq_to_bits_auto(shard, p, auto_noise=True, auto_center=True, halo_given=True, left_halo=halo, pos_base=a, n_total=n)
        rec = sp.message_records(shard, res, p, divisor, pos_base=a, n_total=n)
        return dict(piece=res.piece(), rec=rec, auto=sp.last_auto)
    out, err = M.run_ranks(world, work)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), want_flat, "corrected pass")
    assert all(o["auto"]["noise"] == whole.noise_threshold and o["auto"]["center"] == whole.center for o in out)
    sc.assert_same_records(S.stitch_records([o["rec"] for o in out]), want_rec, "corrected pass")
    msgs = S.message_data([o["piece"] for o in out], [o["rec"] for o in out], p)
    key = lambda m: (list(m.plain_bits), m.pause, list(m.bit_sample_pos), m.timestamp)      # noqa: E731
    assert [key(m) for m in msgs] == [key(m) for m in want_msgs]
    assert all(mc.same_float(a.rssi, b.rssi) for a, b in zip(msgs, want_msgs))             # the RSSI on its bit pattern


# ---- 4. PSK: the hand-over -----------------------------------------------------------------------------------------------------------------
def test_psk_pass_with_automatic_noise_and_center(pipe, engines):
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import costas_halo_samples
    n, world = 240_000, 2
    rng = np.random.default_rng(12)
    ph = np.repeat(np.array([-90, 90])[rng.integers(0, 2, n // 100 + 1)] * np.pi / 180, 100)[:n] + 2 * np.pi * 0.04 * np.arange(n)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1)
    for a in (60_000, 150_000):
        iq[a:a + 6_000] = 0.0                              # gaps of noise alone: some of detect_noise_level's chunks are quiet
    iq = (iq + 0.1 * np.sqrt(0.5) * rng.standard_normal((n, 2))).astype(np.float32)
    p, dev = DemodParams("PSK", 1, 0.0, 0.3, 1.0, 5, 100, 0.1, 8, True), to_dev(iq)
    whole = pipe.iq_to_bits(dev, p, want_qad=True, auto_noise=True, auto_center=True)
    want = single_flat(whole)
    assert whole.noise_threshold > 0 and whole.center is not None and whole.center != p.center
    bounds = bounds_of(n, world)
    halos = [None] + [dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a] for a, _ in bounds[1:]]
    out, err = run_auto(engines, dev, bounds, p, kw_for=lambda r: dict(left_raw=halos[r]), timeout=300, auto_noise=True, auto_center=True)
    assert not any(err), err
    A.assert_flat_equal(stitched(out), want, "psk")
    assert all(o["auto"]["noise"] == whole.noise_threshold and o["center"] == whole.center and o["auto"]["center_detected"] for o in out)


# ---- 5. refusals return and do not hang --------------------------------------------------------------------------------------------------
def test_noise_level_not_below_max_magnitude_raises_on_every_rank(engines):
    dev = to_dev(A.loud_capture(6_400))
    for kw in (dict(auto_noise=True, auto_center=True), dict(auto_noise=True)):
        _, err = run_auto(engines, dev, bounds_of(6_400, 3), A.params("FSK"), timeout=30, runner=A.run_ranks_together, **kw)
        assert all(isinstance(e, ValueError) and "max_magnitude" in str(e) for e in err), err


@pytest.mark.parametrize("auto_noise", [False, True])
def test_non_contiguous_shard_on_one_rank_raises_and_does_not_hang(engines, pass_inputs, auto_noise):
    """the rank whose shard is a strided view raises before it enters a collective; the others leave theirs (a broken barrier)"""
    iq, dev, p, _, _ = pass_inputs("FSK2", np.float32)
    bounds = bounds_of(N_PASS, 3)
    strided = dev[bounds[1][0]:bounds[1][1]].repeat_interleave(2, dim=0)[::2]
    assert not strided.is_contiguous() and strided.shape[0] == bounds[1][1] - bounds[1][0]
    _, err = run_auto(engines, dev, bounds, p, shard_for=lambda r: strided if r == 1 else dev[bounds[r][0]:bounds[r][1]], timeout=60,
                      auto_noise=auto_noise, auto_center=True)
    assert isinstance(err[1], ValueError) and "contiguous" in str(err[1]), err
    assert err[0] is not None and err[2] is not None and not isinstance(err[0], ValueError), err
