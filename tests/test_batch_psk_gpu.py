"""DevicePipeline.iq_to_bits_batch_psk and costas_demod_batch (urh_amd/batch/; include/urhgpu.h "a batch of captures: PSK") against the
oracle: every capture of a batch comes back with the demodulated signal (as uint32, element 0 = -4), pulse table, bits, offsets, pauses
and positions that oracle.afp_demod(.., "PSK", ..) -> grab_pulse_lens -> ppseq_to_bits_flat give for that capture alone, whatever shares
its wavefront; with automatic noise, automatic center and records, what the single pass iq_to_bits gives on that capture alone.  The
kernel's boundaries are the tile of 64 samples, the wavefront of 64 captures and n <= 2.  The exactness tests run with cap_rows="bound"
and assert that no capture was truncated."""
from dataclasses import replace

import numpy as np
import pytest

import batch_psk_cases as P
from conftest import GOLDEN_CASES, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def run_exact(pipe, oracle, caps, p, want_qad=True, nan=(), **kw):
    res = pipe.iq_to_bits_batch_psk(caps, p, want_qad=want_qad, cap_rows="bound", **kw)
    assert len(res) == len(caps) and res.truncated == []
    for i, iq in enumerate(caps):
        assert res[i].n_samples == len(iq) and res[i].seq == i
        P.same(res[i], P.reference(oracle, iq, p), res.qad(i) if want_qad else None, (i, len(iq)), nan_payloads=i not in nan)
    return res


def got_of(h):
    return [np.array(x) for x in (h.ppseq(), h.bits(), h.msg_off, h.pauses, h.bit_sample_pos(), h.pos_offsets())]


def single_pass(pipe, iq, p, **kw):
    """the capture alone through iq_to_bits: (BitsResult, its HostBits)"""
    one = pipe.iq_to_bits(P.to_dev(pipe, iq), replace(p, write_bit_sample_pos=True), want_qad=True, cap_rows=len(iq) // (p.tolerance + 1) + 2, **kw)
    return one, one.host(pool={})


def same_as_pass(got, qad, h, one, tag):
    for x, y in zip(got, got_of(h)):
        assert np.array_equal(x, y), tag
    if qad is not None:
        assert np.array_equal(qad.view(np.uint32), one.qad.cpu().numpy()[:len(qad)].view(np.uint32)), tag


# ---- 1. lengths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,bps", [(2, 1), (4, 2), (4, 3)])
def test_lengths_around_the_tile_and_the_single_pass_kernels(pipe, oracle, order, bps):
    lengths = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 4097, 8192, 8193, 12_289]
    perm = np.random.default_rng(order + bps).permutation(len(lengths))
    caps = [P.gapped(lengths[i], order, seed=100 * order + int(i))[0] for i in perm]
    p = P.params(order, 0.2, bps=bps)
    res = run_exact(pipe, oracle, caps, p)
    # 8192 / 8193: where the single-capture pass switches between its serial and its speculative kernel
    kept = [(i, got_of(res[i]), res.qad(i).cpu().numpy()) for i, c in enumerate(caps) if len(c) in (8192, 8193)]
    assert len(kept) == 2
    for i, got, qad in kept:
        one, h = single_pass(pipe, caps[i], p)
        same_as_pass(got, qad, h, one, ("pass", len(caps[i])))


# ---- 2. number of captures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 130, 2000])
def test_many_captures(pipe, oracle, k):
    rng = np.random.default_rng(k)
    pool, noise = P.psk_capture(40_000, 4, seed=k, gaps=[(a, a + 120) for a in range(700, 40_000, 1900)])
    lengths = rng.integers(0, 301, k)
    at = rng.integers(0, 39_000, k)
    caps = [np.ascontiguousarray(pool[a:a + n]) for a, n in zip(at, lengths)]
    res = run_exact(pipe, oracle, caps, P.params(4, noise, tolerance=2), want_qad=(k != 2000))
    assert len(res) == k
    if k == 0:
        assert list(res) == [] and res.check() is res


# ---- 3. contents --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("noise,bandwidth", [(0.0, 0.1), (0.2, 0.05), (0.2, 0.1), (0.2, 0.3)])
def test_contents(pipe, oracle, order, noise, bandwidth):
    T, n = P.TILE, 3001
    cap = lambda seed, gaps: P.psk_capture(n, order, seed, gaps=gaps)[0]          # noqa: E731
    rng = np.random.default_rng(order)
    caps = [
        cap(1, ((0, 500),)), cap(2, ((n - 444, n),)),                                  # a leading gap, a trailing gap
        cap(3, ((1000, 1000 + 3 * T + 17),)),                                          # a gap that spans three tiles
        cap(4, ((5 * T - 1, 5 * T - 1 + 63),)), cap(5, ((7 * T - 1, 7 * T - 1 + 64),)), cap(6, ((9 * T - 1, 9 * T - 1 + 65),)),
        np.zeros((1501, 2), np.float32),                                               # all zero
        (0.3 * rng.standard_normal((2001, 2))).astype(np.float32),                     # noise only
        cap(7, ()),
    ]
    run_exact(pipe, oracle, caps, P.params(order, noise, bandwidth))


# ---- 4. sample types ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.int8, np.uint8, np.int16, np.uint16], ids=lambda d: np.dtype(d).name)
def test_sample_types_at_odd_offsets(pipe, oracle, order, dtype):
    """captures of odd length in front: the later ones start off 16-byte (int8: off 4-byte) alignment"""
    made = [P.gapped(n, order, seed=n, dtype=dtype) for n in (1, 3, 777, 5, 2049, 1, 4095, 64, 129)]
    run_exact(pipe, oracle, [iq for iq, _ in made], P.params(order, made[0][1]))


# ---- 5. neighbours ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
def test_the_neighbours_do_not_matter(pipe, oracle, order):
    """one wavefront's lanes: the same capture at positions 0, 2 and 5, between them a loud capture, a 63-sample all-zero one and the
    capture with a NaN in its gap, which takes the whole wavefront through the exact step from its sample on"""
    import edge_inputs as E
    nan_iq, noise, at = E.psk_nan_in_gap(order, n=8000)
    x = P.gapped(3001, order, seed=5)[0]
    loud = (3.0 * np.random.default_rng(0).standard_normal((555, 2))).astype(np.float32)
    caps = [x, loud, x, np.zeros((63, 2), np.float32), nan_iq, x]
    res = run_exact(pipe, oracle, caps, P.params(order, noise), nan=(4,))
    for i in (2, 5):
        assert np.array_equal(res[i].ppseq(), res[0].ppseq()) and np.array_equal(res[i].bits(), res[0].bits())
        assert np.array_equal(res.qad(i).cpu().numpy().view(np.uint32), res.qad(0).cpu().numpy().view(np.uint32))
    q = res.qad(4).cpu().numpy()
    # poisoned from its sample on (the gated samples behind it still give -4), and no earlier
    assert not np.isnan(q[:at]).any() and np.isnan(q[at]) and np.isnan(q[-1]) and np.isin(q[at:][~np.isnan(q[at:])], [-4.0]).all()


# ---- 6. reference fixtures ----------------------------------------------------------------------------------------------------------------
PSK_FIXTURES = [c for c in GOLDEN_CASES if load_golden(c)["modulation_type"] == "PSK"]


@pytest.mark.parametrize("name", PSK_FIXTURES)
def test_reference_fixtures(pipe, oracle, name):
    """[capture, its first half, capture] with the fixture's own parameters: entries 0 and 2 equal what the real reference recorded (its
    element 0 is unwritten memory: compared from index 1)"""
    from urh_amd.pipeline import DemodParams
    g = load_golden(name)
    p = DemodParams("PSK", g["bits_per_symbol"], g["noise_threshold"], g["center"], g["center_spacing"], g["tolerance"], g["samples_per_symbol"],
                    g["costas_loop_bandwidth"], g["pause_threshold"], False)
    iq = g["iq"]
    half = np.ascontiguousarray(iq[:len(iq) // 2])
    res = pipe.iq_to_bits_batch_psk([iq, half, iq], p, want_qad=True, cap_rows="bound", long_from=2 ** 31 - 1)
    assert res.truncated == []
    whole = P.reference(oracle, iq, p)
    for i in (0, 2):
        h = res[i]
        assert np.array_equal(res.qad(i).cpu().numpy()[1:].view(np.uint32), g["qad"][1:].view(np.uint32))
        # the recorded table's FIRST state is that of the unwritten element (about -2.8e29 in the recorded runs: a data state, where the
        # library's documented -4 is a pause); its length and every other row, the bits, offsets, pauses and positions are the record's
        assert np.array_equal(h.ppseq()[1:], g["ppseq"][1:]) and np.array_equal(h.ppseq()[:, 1], g["ppseq"][:, 1]) and h.ppseq()[0, 0] == -1
        P.same(h, whole, res.qad(i), (name, i))
        assert np.array_equal(h.bits(), g["bits"]) and np.array_equal(h.msg_off, g["msg_off"]) and np.array_equal(h.pauses, g["pauses"])
        assert np.array_equal(h.bit_sample_pos(), g["pos"]) and np.array_equal(h.pos_offsets(), g["pos_off"])
    P.same(res[1], P.reference(oracle, half, p), res.qad(1), name)


def test_there_are_psk_fixtures():
    """a guard against an empty parametrisation above; it says nothing about the feature"""
    assert PSK_FIXTURES


# ---- 7. / 8. automatic noise, automatic center ---------------------------------------------------------------------------------------------
def session(order, n=6001):
    """captures whose gains differ by 20 dB, each with quiet stretches for the noise floor; shared by the tests below, never changed"""
    x = P.psk_capture(n, order, seed=70 + order, gaps=((0, 700), (n // 2, n // 2 + 900)))[0]
    y = P.psk_capture(n - 1300, order, seed=71 + order, gaps=((2000, 2600),))[0]
    return [x, (x * np.float32(0.1)).astype(np.float32), y, (y * np.float32(0.1)).astype(np.float32), np.ascontiguousarray(x[:777])]


def check_against_the_pass(pipe, caps, p, auto_noise, auto_center, divisor=None, **kw):
    res = pipe.iq_to_bits_batch_psk(caps, p, auto_noise=auto_noise, auto_center=auto_center, message_length_divisor=divisor, want_qad=True, cap_rows="bound", **kw)
    assert len(res) == len(caps)
    flags = res.noise_flags if auto_noise else [1] * len(caps)
    kept = []
    for i in range(len(caps)):
        if flags[i] == 0:
            with pytest.raises((ValueError, OverflowError)):
                res[i]
            kept.append(None)
            continue
        assert res[i].truncated == 0
        kept.append((got_of(res[i]), res.qad(i).cpu().numpy(), res[i].n_samples, None if divisor is None else np.array(res[i].records),
                     None if divisor is None else res.message_data(i, 2e6, 3.5)))
    noise, centers, cflags = res.noise, res.centers, res.center_flags
    for i, iq in enumerate(caps):                                # (the pipeline's next passes: the batch's views were copied above)
        if kept[i] is None:
            continue
        got, qad, n_samples, rec, msgs = kept[i]
        one, h = single_pass(pipe, iq, p, auto_noise=auto_noise, auto_center=auto_center, msg_records=divisor is not None, message_length_divisor=divisor or 1)
        tag = (i, len(iq), auto_noise, auto_center, divisor)
        assert h.n_samples == n_samples, tag
        same_as_pass(got, qad, h, one, tag)
        if auto_noise:
            assert one.noise_flag == flags[i] and float(one.noise_threshold).hex() == float(noise[i]).hex(), tag
        if auto_center:
            assert one.center == centers[i] and one.center_flag == cflags[i], (tag, one.center, centers[i], one.center_flag, cflags[i])
        if divisor is not None:
            want_rec = one.records
            assert len(rec) == len(want_rec), tag
            for f in ("first_pos", "mid_pos", "n_pad", "flag"):
                assert np.array_equal(rec[f], want_rec[f]), (tag, f)
            assert np.array_equal(np.ascontiguousarray(rec["rssi"]).view(np.uint64), np.ascontiguousarray(want_rec["rssi"]).view(np.uint64)), tag
            want = one.message_data(2e6, 3.5)
            assert len(msgs) == len(want), tag
            for a, b in zip(msgs, want):
                assert list(a.plain_bits) == list(b.plain_bits) and a.pause == b.pause and list(a.bit_sample_pos) == list(b.bit_sample_pos), tag
                assert np.float64(a.rssi).view(np.uint64) == np.float64(b.rssi).view(np.uint64) and a.timestamp == b.timestamp, tag
    return res, kept


@pytest.mark.parametrize("order", [2, 4])
def test_automatic_noise(pipe, order):
    n = 6001
    rng = np.random.default_rng(order)
    infs = np.array(session(order)[0])
    infs[::50, 0] = np.inf                                                          # the reference raises: math.ceil of an infinity
    gates_all = (3.0 * P.psk_capture(n, order, seed=9)[0] + 1.5 * rng.standard_normal((n, 2))).astype(np.float32)
    caps = session(order) + [gates_all, infs, session(order)[2]]
    p = P.params(order, 0.0)
    res, kept = check_against_the_pass(pipe, caps, p, True, False)
    assert res.noise_flags[:5] == [1] * 5 and res.noise_flags[5:] == [2, 0, 1], res.noise_flags
    assert res.noise[0] > 3 * res.noise[1] and res.noise[2] > 3 * res.noise[3]      # 20 dB apart in gain: each gated with its own
    # a capture gated entirely: the reference's zeros(2)
    assert kept[5][2] == 2 and np.array_equal(kept[5][1], np.zeros(2, np.float32))
    with pytest.raises(OverflowError):
        res[6]
    levels = pipe.detect_noise_levels([c for i, c in enumerate(caps) if i != 6])
    assert [float(v).hex() for v in levels] == [float(v).hex() for i, v in enumerate(res.noise) if i != 6]


@pytest.mark.parametrize("auto_noise", [False, True])
@pytest.mark.parametrize("order", [2, 4])
def test_automatic_center(pipe, order, auto_noise):
    """no bound on how many captures the device leaves to numpy: those are sliced again and must come out equal too"""
    caps = session(order)
    p = P.params(order, 0.02)
    res, _ = check_against_the_pass(pipe, caps, p, auto_noise, True)
    assert len(res.centers) == len(caps) and any(c is not None for c in res.centers)


# ---- 9. records ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", [1, 8])
def test_records(pipe, divisor):
    from urh_amd import protocol
    caps = session(4)
    p = P.params(4, 0.02)
    res, kept = check_against_the_pass(pipe, caps, p, False, False, divisor)
    assert sum(len(k[4]) for k in kept) >= len(caps)                                 # (the session has messages)
    got = protocol.get_protocols_from_signals_dev(pipe, caps, p, divisor, sample_rate=2e6, timestamps=[3.5] * len(caps), cap_rows="bound")
    assert len(got) == len(caps)
    for i, msgs in enumerate(got):
        want = kept[i][4]
        assert len(msgs) == len(want)
        for a, b in zip(msgs, want):
            assert list(a.plain_bits) == list(b.plain_bits) and a.pause == b.pause and list(a.bit_sample_pos) == list(b.bit_sample_pos)
            assert np.float64(a.rssi).view(np.uint64) == np.float64(b.rssi).view(np.uint64) and a.timestamp == b.timestamp


def test_records_with_automatic_noise_and_center(pipe):
    check_against_the_pass(pipe, session(2), P.params(2, 0.0), True, True, 8)


# ---- 10. launches and copies ---------------------------------------------------------------------------------------------------------------
def test_launches_and_copies_do_not_depend_on_the_batch(pipe):
    """the header's numbers: 4 launches (Costas, walk, scan, pack) and 2 copies (directory, blobs); with automatic noise and a center in one
    group 5 + 14 launches and 4 copies (the noise blocks, the center blocks) -- for 3 captures and for 2000"""
    from urh_amd import _lib, batch
    x = session(4)[0][:1500]
    p = P.params(4, 0.02)
    group = batch.batch_center_plan([0], None, int(_lib.load().urhgpu_center_hist_cap(pipe.ctx.handle)))[2]
    assert group >= 2000
    for kw, want in (({}, (4, 2)), ({"auto_noise": True, "auto_center": True}, (5 + 14, 4))):
        spent = []
        for k in (3, 2000):
            before = batch.launch_counts(pipe)
            res = pipe.iq_to_bits_batch_psk([x] * k, p, **kw)
            after = batch.launch_counts(pipe)
            assert len(res) == k
            if kw:                                           # (a center the device decides: no second slicing, whose launches are counted too)
                assert set(res.center_flags) == {1}, set(res.center_flags)
            spent.append((after[0] - before[0], after[1] - before[1]))
        assert spent[0] == spent[1] == want, (kw, spent)


# ---- 11. routing and retry -----------------------------------------------------------------------------------------------------------------
def test_a_long_capture_is_routed_through_a_pass(pipe, oracle):
    import torch
    caps = [P.gapped(n, 4, seed=n)[0] for n in (3001, 70_001, 0, 4999)]
    p = P.params(4, 0.2)
    want = [P.reference(oracle, c, p) for c in caps]
    res = pipe.iq_to_bits_batch_psk(caps, p, want_qad=True, cap_rows="bound", long_from=50_000)
    assert len(res) == 4 and res.truncated == []
    for i in range(4):
        P.same(res[i], want[i], res.qad(i), ("numpy", i))
    # ... and as device tensors, and already packed
    dev = [torch.from_numpy(c).cuda() for c in caps]
    got = pipe.iq_to_bits_batch_psk(dev, p, want_qad=True, cap_rows="bound", long_from=50_000)
    for i in range(4):
        P.same(got[i], want[i], got.qad(i), ("tensors", i))
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])])
    packed = pipe.iq_to_bits_batch_psk((torch.cat(dev), starts), p, want_qad=True, cap_rows="bound", long_from=2 ** 31 - 1)
    for i in range(4):
        P.same(packed[i], want[i], packed.qad(i), ("packed", i))


def test_a_capture_that_outgrows_its_region(pipe, oracle):
    """the default policy: noise makes more rows than the stream's formula holds; rows_needed says how many, retry(k) completes it"""
    from urh_amd import _lib
    p = P.params(4, 0.0, tolerance=1)
    noise = (0.3 * np.random.default_rng(1).standard_normal((20_000, 2))).astype(np.float32)
    caps = [P.gapped(5001, 4, seed=1)[0], noise, P.gapped(7001, 4, seed=2)[0]]
    want = [P.reference(oracle, c, p) for c in caps]
    assert len(want[1][1]) > 864
    res = pipe.iq_to_bits_batch_psk(caps, p, want_qad=True)
    assert 1 in res.truncated
    h = res[1]
    assert h.truncated & 1 and h.rows_needed == len(want[1][1]) and h.n_rows == 864
    assert np.array_equal(h.ppseq(), want[1][1][:864])
    with pytest.raises(_lib.UrhGpuError):
        h.check()
    for k in list(res.truncated):
        again = res.retry(k)
        assert again is res[k]
    assert res.truncated == []
    for i in range(3):                                                         # (the retries left the others' views alone)
        P.same(res[i], want[i], res.qad(i), ("after retry", i))


# ---- 12. the Costas launch alone -----------------------------------------------------------------------------------------------------------
def test_costas_demod_batch_alone(pipe, oracle):
    caps = session(4) + [np.zeros((0, 2), np.float32), session(4)[0][:2]]
    p = P.params(4, 0.02)
    qad, starts = pipe.costas_demod_batch(caps, p)
    assert len(starts) == len(caps) + 1 and int(starts[-1]) == sum(len(c) for c in caps) == qad.shape[0]
    host = qad.cpu().numpy()
    for i, iq in enumerate(caps):
        assert np.array_equal(host[starts[i]:starts[i + 1]].view(np.uint32), P.reference(oracle, iq, p)[0].view(np.uint32)), i
    # one threshold per capture
    noise = [0.02, 0.002, 0.05, 0.0, 0.3, 0.1, 0.1]
    qad_n, _ = pipe.costas_demod_batch(caps, p, noise=noise)
    host = qad_n.cpu().numpy()
    for i, iq in enumerate(caps):
        assert np.array_equal(host[starts[i]:starts[i + 1]].view(np.uint32), P.reference(oracle, iq, replace(p, noise_threshold=noise[i]))[0].view(np.uint32)), i
    # the shape detect_centers takes: the centers of the batch with automatic center
    centers = pipe.detect_centers((qad, starts))
    res = pipe.iq_to_bits_batch_psk(caps, p, auto_center=True)
    assert centers == res.centers


def test_costas_demod_batch_calls_back_to_back(pipe, oracle):
    """the launch alone returns without waiting: three calls with device tensors of different lengths and thresholds, nothing synchronised
    in between -- the first one's loop runs for tens of milliseconds, so the later uploads are still queued when the host goes on -- and
    every call's result is its own captures' (a staging buffer is not rewritten while a queued upload has yet to read it)"""
    p = P.params(4, 0.2)
    sessions = [[P.gapped(n, 4, seed=300 + 10 * j + i)[0] for i, n in enumerate(lengths)]
                for j, lengths in enumerate(((70_001, 900, 4097), (129, 3001, 64, 2049, 5), (5000, 0, 777)))]
    noises = [None, [0.2, 0.0, 0.05, 0.3, 0.2], [0.1, 0.2, 0.02]]
    dev = [[P.to_dev(pipe, c) for c in caps] for caps in sessions]
    import torch
    torch.cuda.synchronize()
    got = [pipe.costas_demod_batch(d, p, noise=nz) for d, nz in zip(dev, noises)]        # (no .cpu(), no synchronize between the calls)
    for j, ((qad, starts), caps) in enumerate(zip(got, sessions)):
        host = qad.cpu().numpy()
        assert len(starts) == len(caps) + 1
        for i, iq in enumerate(caps):
            q = p if noises[j] is None else replace(p, noise_threshold=noises[j][i])
            assert np.array_equal(host[starts[i]:starts[i + 1]].view(np.uint32), P.reference(oracle, iq, q)[0].view(np.uint32)), (j, i)
