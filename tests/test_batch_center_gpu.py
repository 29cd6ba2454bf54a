"""DevicePipeline.iq_to_bits_batch_center, detect_centers and qad_to_bits_batch (urh_amd/batch/, urh_amd/csrc/batch_center.hip;
include/urhgpu.h "a batch of captures: automatic center per capture") against the oracle: every capture of a batch comes back with the
center detect_center gives for its own demodulated signal and with the pulse table, bits, offsets, pauses, positions and demodulated
signal of the reference sliced with THAT center, whatever lies beside it in the buffer -- and with what DevicePipeline.iq_to_bits(...,
auto_center=True) gives on it alone.  The class the device REPORTS for a capture (decided / none / wide / tie) is the one numpy expects
(center_cases.expected), so that no capture passes through a host fallback unnoticed."""
import collections
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import batch_auto_cases as bac
import batch_center_cases as B
import batch_edge_cases as BE
import center_cases as cc
import noise_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def got_of(h):
    return h.ppseq(), h.bits(), h.msg_off, h.pauses, h.bit_sample_pos(), h.pos_offsets()


def same(res, i, r, tag, want_qad=True, nan_payloads=True):
    """capture i of the batch against reference r = (threshold, noise flag, (center, qad, table, bits, ...)); nan_payloads=False: where both
    demodulated signals hold a NaN its payload is not compared (edge_inputs.same_bits: the capture with a NaN sample)"""
    thr, nflag, ref = r
    h = res[i]
    assert h.truncated == 0 and h.rows_needed == len(ref[2]) and h.seq == i, (tag, h.truncated, h.rows_needed, len(ref[2]))
    if res.noise is not None:
        assert res.noise_flags[i] == nflag and res.noise[i].hex() == float(thr).hex(), (tag, res.noise[i], thr)
    assert h.n_samples == len(ref[1]), tag
    cc.assert_equal(res.centers[i], res.qad(i).cpu().numpy() if (want_qad and nan_payloads) else None, got_of(h), ref, tag)
    if want_qad and not nan_payloads:
        import edge_inputs as E
        got = res.qad(i).cpu().numpy()
        assert got.shape == ref[1].shape and E.same_bits(got[1:], ref[1][1:]).all(), tag


def check_batch(pipe, oracle, caps, p, max_size, key, auto_noise=True, pool_bins=cc.POOL_BINS, alone=None, twins=None):
    """the whole batch against the oracle; the reported classes; `alone`: these captures against the single pass too.  Returns the classes."""
    import torch
    res = pipe.iq_to_bits_batch_center(caps, p, auto_noise=auto_noise, center_max_size=max_size, want_qad=True, cap_rows="bound")
    assert len(res) == len(caps) and res.truncated == []
    classes = []
    for i, iq in enumerate(caps):
        r = B.reference(oracle, iq, p, max_size, auto_noise, key=(key, i))
        cls = B.expected_class(r, max_size, pool_bins)
        classes.append(cls)
        assert res.center_flags[i] == cc.FLAG[cls], (key, i, len(iq), cls, res.center_flags[i])
        same(res, i, r, (key, i, len(iq), max_size, cls))
    if twins:
        a, b = got_of(res[twins[0]]), got_of(res[twins[1]])
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and res.centers[twins[0]] == res.centers[twins[1]]
    kept = [(i, res.centers[i], res.center_flags[i], [np.array(x) for x in got_of(res[i])]) for i in (alone or [])]
    for i, center, flag, got in kept:                            # (the pipeline's next pass: the batch's views were copied above)
        iq = caps[i]
        one = pipe.iq_to_bits(torch.from_numpy(np.array(iq)).to(pipe.device), replace(p, write_bit_sample_pos=True), auto_noise=auto_noise, auto_center=True,
                              center_max_size=max_size, cap_rows=len(iq) // (p.tolerance + 1) + 2)
        h = one.host(pool={})
        assert one.center == center and one.center_flag == flag, (key, i, one.center, center, one.center_flag, flag)
        for x, y in zip(got_of(h), got):
            assert np.array_equal(x, y), (key, i)
    return classes


@pytest.mark.parametrize("dtype", B.GAIN_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mod", B.GAIN_MODS)
def test_gain_sweep(pipe, oracle, mod, dtype):
    name = np.dtype(dtype).name
    sweep = B.gain_sweep(mod, dtype)
    caps = [sweep[0]] + sweep + [sweep[0]]                       # a clean capture first and last: identical results
    p = B.gain_params(mod)
    seen = collections.Counter()
    for max_size in B.GAIN_MAX_SIZES:
        classes = check_batch(pipe, oracle, caps, p, max_size, ("gain", mod, name), alone=range(len(caps)), twins=(0, len(caps) - 1))
        seen.update(classes[1:-1])
    assert dict(seen) == B.GAIN_CLASSES[(mod, name)]


def test_gain_sweep_with_a_small_pool_reports_wide(oracle):
    from urh_amd.pipeline import DevicePipeline
    small = DevicePipeline(0, tuning={"auto_center_max_bins": 64})
    caps = B.gain_sweep("FSK", np.float32)
    classes = check_batch(small, oracle, caps, B.gain_params("FSK"), None, ("gain", "FSK", "float32-pool64"), pool_bins=64, alone=range(128))
    assert classes.count("wide") >= 10 and classes.count("ok") >= 10, collections.Counter(classes)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mod", cc.MODS)
def test_geometry_sweep(pipe, oracle, mod, dtype):
    caps = B.geometry_sweep(dtype)
    p = B.geometry_params(mod, dtype)
    for max_size in cc.MAX_SIZES:
        check_batch(pipe, oracle, caps, p, max_size, ("geometry", mod, np.dtype(dtype).name), alone=[i for i, c in enumerate(caps) if len(c) >= 1],
                    twins=(0, len(caps) - 1))


@pytest.mark.parametrize("mod,dtype", [("FSK", np.float32), ("FSK", np.int8), ("FSK", np.uint8), ("ASK", np.float32), ("ASK", np.int16)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_with_the_configured_noise_threshold(pipe, oracle, mod, dtype):
    """auto_noise=False: every capture gated with p.noise_threshold (center_cases.noise_threshold: the gaps are gated, compaction and the
    first-sample skip are exercised; unsigned: nothing is gated)"""
    caps = B.geometry_sweep(dtype)
    p = B.geometry_params(mod, dtype)
    seen = collections.Counter()
    for max_size in (None, 1000, 127):
        seen.update(check_batch(pipe, oracle, caps, p, max_size, ("geometry-cfg", mod, np.dtype(dtype).name), auto_noise=False,
                                alone=[i for i, c in enumerate(caps) if len(c) >= 1], twins=(0, len(caps) - 1)))
    assert seen["ok"] >= 10
    plain = pipe.iq_to_bits_batch_center(caps[:3], p, auto_noise=False)
    assert plain.noise is None and plain.noise_flags is None and len(plain.centers) == 3


def test_special_batches(pipe, oracle):
    p = nc.params("FSK", 1, write_pos=False)
    caps = B.first_sample_batch()
    check_batch(pipe, oracle, caps, cc.params("FSK", np.float32, write_pos=False), None, "first-sample", auto_noise=False, alone=range(len(caps)), twins=(0, 5))
    caps = B.noise_between_batch()
    check_batch(pipe, oracle, caps, p, None, "noise-between", alone=range(len(caps)), twins=(0, 2))
    caps = B.seam_batch()
    pa = nc.params("ASK", 1, write_pos=False)
    check_batch(pipe, oracle, caps, pa, None, "seam", alone=range(len(caps)))
    centers = [c for c in pipe.iq_to_bits_batch_center(caps, pa).centers if c is not None]
    assert len(centers) >= 2 and max(centers) > 3 * min(centers)                                        # (no single center serves them)


@pytest.mark.parametrize("k", B.TINY_KS)
def test_many_tiny_captures(pipe, oracle, k):
    caps = B.tiny_batch(k)
    check_batch(pipe, oracle, caps, B.tiny_params(), None, ("tiny", k), auto_noise=False, alone=[i for i, c in enumerate(caps) if len(c) >= 1])


def test_detect_centers_and_qad_to_bits_batch_alone(pipe, oracle):
    from urh_amd import batch
    p = B.gain_params("FSK")
    caps = B.gain_sweep("FSK", np.float32)[::3]
    refs = [B.reference(oracle, iq, p, None, True, key=("alone", i)) for i, iq in enumerate(caps)]
    qads = [r[2][1] for r in refs]
    cat = np.concatenate(qads)
    starts = np.concatenate([[0], np.cumsum([len(q) for q in qads])])
    for max_size in (None, 1000):
        centers, flags = batch.detect_centers(pipe, (cat, starts), max_size, return_flags=True)
        assert centers == pipe.detect_centers((cat, starts), max_size)
        for i, q in enumerate(qads):
            c = oracle.detect_center(q, max_size)
            assert (c is None and centers[i] is None) or float(c) == centers[i], (i, c, centers[i])
            assert flags[i] == cc.FLAG[cc.expected(q, max_size)], i
    want = [r[2][0] for r in refs]
    res = pipe.qad_to_bits_batch((cat, starts), p, centers=want, cap_rows="bound")
    plain = None
    for i, r in enumerate(refs):
        assert np.array_equal(res[i].ppseq(), r[2][2]) and np.array_equal(res[i].bits(), r[2][3]) and np.array_equal(res[i].msg_off, r[2][4]), i
        assert np.array_equal(res[i].pauses, r[2][5]) and np.array_equal(res[i].bit_sample_pos(), r[2][6]), i
    plain = pipe.qad_to_bits_batch((cat, starts), p, cap_rows="bound")             # p.center for every capture
    differs = 0
    for i, q in enumerate(qads):
        pp, flat = nc.slice_qad(oracle, q, p)
        assert np.array_equal(plain[i].ppseq(), pp) and np.array_equal(plain[i].bits(), flat[0]) and np.array_equal(plain[i].pauses, flat[2]), i
        differs += not np.array_equal(pp, refs[i][2][2])
    assert differs > 0


def _by_class(oracle, mod, classes, n=1033):
    """captures of the float32 gain sweep with n samples that numpy classes as one of `classes` (max_size None)"""
    p = B.gain_params(mod)
    out = []
    for i, iq in enumerate(B.gain_sweep(mod, np.float32)):
        if len(iq) == n and B.expected_class(B.reference(oracle, iq, p, None, True, key=("gain", mod, "float32", i + 1)), None) in classes:
            out.append(iq)
    return out


def test_launches_and_copies_do_not_depend_on_the_number_of_captures(pipe, oracle):
    """5 + 14 ceil(K / group) launches and 4 copies with automatic noise (noise, demodulation, per group the chain's 13 and the publish step,
    walk, scan, pack; directory, blobs, noise blocks, center blocks); a batch with ties: 3 launches and 3 copies more (the pool's fetch; walk,
    scan, pack; directory, blobs), whatever the number of ties"""
    from urh_amd import batch, _lib
    p = B.gain_params("FSK")
    plain = _by_class(oracle, "FSK", ("ok", "none"))
    tied = _by_class(oracle, "FSK", ("tie",))
    assert len(plain) >= 3 and len(tied) >= 5
    group = batch.batch_center_plan([0], None, int(_lib.load().urhgpu_center_hist_cap(pipe.ctx.handle)))[2]
    assert group == 4096
    for k, ties in ((3, 0), (5000, 0), (60, 5), (120, 50)):
        caps = [plain[i % len(plain)] for i in range(k - ties)] + [tied[i % len(tied)] for i in range(ties)]
        before = batch.launch_counts(pipe)
        res = pipe.iq_to_bits_batch_center(caps, p)
        after = batch.launch_counts(pipe)
        groups = -(-k // group)
        extra = 3 if ties else 0
        assert (after[0] - before[0], after[1] - before[1]) == (5 + 14 * groups + extra, 4 + extra), (k, ties)
        assert sum(f == 3 for f in res.center_flags) == ties and set(res.center_flags) <= {0, 1, 3}
        if k == 5000:
            assert groups == 2 and res.centers[4999] == res.centers[4999 % len(plain)] and res.centers[4096] == res.centers[4096 % len(plain)]
    before = batch.launch_counts(pipe)
    pipe.iq_to_bits_batch_center(plain[:3], p, auto_noise=False)
    after = batch.launch_counts(pipe)
    assert (after[0] - before[0], after[1] - before[1]) == (4 + 14, 3)


def test_routing_by_long_from(pipe, oracle):
    p = nc.params("ASK", 1, write_pos=False)
    caps = [nc.capture(7400 + i, n, "ASK", 1, np.float32, s, a) for i, (n, (s, a)) in enumerate(zip((4999, 5000, 900, 5001, 12_801), nc.STREAM_GAINS))]
    refs = [B.reference(oracle, c, p, 1000, True, key=("routing", i)) for i, c in enumerate(caps)]
    whole = pipe.iq_to_bits_batch_center(caps, p, center_max_size=1000, want_qad=True, cap_rows="bound", long_from=2 ** 31 - 1)
    centers, flags = list(whole.centers), list(whole.center_flags)
    for i, r in enumerate(refs):
        same(whole, i, r, ("batch", i))
    routed = pipe.iq_to_bits_batch_center(caps, p, center_max_size=1000, want_qad=True, cap_rows="bound", long_from=5000)
    assert routed.centers == centers and routed.center_flags == flags and routed.noise_flags == [1] * 5
    for i, r in enumerate(refs):
        same(routed, i, r, ("routed", i))
    assert len({c for c in centers if c is not None}) > 1


def test_truncation_and_retry(pipe, oracle):
    p = B.gain_params("FSK")
    sweep = B.gain_sweep("FSK", np.float32)
    caps = [sweep[i] for i in (1, 2, 3, 17)]
    refs = [B.reference(oracle, c, p, None, True, key=("trunc", i)) for i, c in enumerate(caps)]
    res = pipe.iq_to_bits_batch_center(caps, p, want_qad=True, cap_rows=2)
    short = [j for j, r in enumerate(refs) if len(r[2][2]) > 2]
    assert res.truncated == short and len(short) >= 2
    for j, r in enumerate(refs):
        assert res[j].rows_needed == len(r[2][2]) and res.centers[j] == r[2][0]
        if j in short:
            assert res[j].truncated & 1 and np.array_equal(res[j].ppseq(), np.asarray(r[2][2]).reshape(-1, 2)[:2])
    k = short[0]
    again = res.retry(k)
    assert res[k] is again and k not in res.truncated
    cc.assert_equal(res.centers[k], res.qad(k).cpu().numpy(), got_of(again), refs[k][2], ("retry", k))


def test_a_tie_pool_that_is_too_small_still_gives_the_right_results(pipe, oracle):
    from urh_amd import batch
    p = B.gain_params("FSK")
    tied = _by_class(oracle, "FSK", ("tie",))[:6]
    res = batch.iq_to_bits_batch_center(pipe, tied, p, want_qad=True, cap_rows="bound", _cap_tie=70)     # (room for one histogram, perhaps two)
    assert res.center_flags == [3] * len(tied)
    for i, iq in enumerate(tied):
        same(res, i, B.reference(oracle, iq, p, None, True, key=("tiepool", i)), ("tiepool", i))


def test_noise_flags_inside_a_batch(pipe, oracle):
    """batch_auto_cases.flag_captures_f32, all seven: noise flags 0 and 2 inside a batch, the others handed out -- among them the constant
    envelope (noise flag 1, threshold 0): its demodulated signal is constant to a few ulp and detect_center's histogram has 166 million
    bins, far more than the pool: the device reports flag 2 and the host's single-range estimator settles the center.  The oracle's
    detect_center takes a minute over that capture, so ITS reference is the real reference's record (threshold, center, class and bit hash
    in tests/golden/batch_center/batch_center.json "flags") with the oracle's demodulation and slicing at that center; the golden record
    is held against every other capture too.  Measured: 8.6 s for this batch on an MI355X, all of it the host's estimator on that one
    histogram (the single pass on the capture alone takes the same 8.6 s: not compared here, it would double the test)."""
    p = nc.params("FSK", 1, write_pos=False)
    golden = B.load_golden()["flags"]
    named = bac.flag_captures_f32()
    caps = [np.ascontiguousarray(c) for _, c in named]
    res = pipe.iq_to_bits_batch_center(caps, p, want_qad=True, cap_rows="bound")
    assert [n for n, _ in named] == ["clean", "zeros", "constant", "one-nan", "inf", "gates-all", "clean-again"]
    assert res.noise_flags == [1, 1, 1, 1, 0, 2, 1] and res.center_flags == [3, 0, 2, 1, res.center_flags[4], 0, 3]
    for i, (name, iq) in enumerate(named):
        g = golden[name]
        if name == "constant":
            thr, center = float.fromhex(g["noise"]), float.fromhex(g["center"])
            qad, pp, flat = nc.reference(oracle, iq, replace(p, write_bit_sample_pos=True), thr, center)
            r = (thr, 1, (center, qad, pp) + tuple(flat))
            assert g["class"] == "wide" and thr == 0.0 and len(set(np.round(qad[1:].astype(np.float64), 5))) == 1      # constant: 2 pi / 100
        else:
            r = B.reference(oracle, iq, p, None, True, key=("flags", name))
        assert r[1] == res.noise_flags[i], name
        if r[1] == 0:
            assert g["noise"] == "OverflowError"
            with pytest.raises(OverflowError):
                res[i]
            continue
        same(res, i, r, name, nan_payloads=name != "one-nan")
        assert res.noise[i].hex() == float.fromhex(g["noise"]).hex(), name
        assert (res.centers[i] is None and g["center"] is None) or res.centers[i].hex() == float.fromhex(g["center"]).hex(), (name, res.centers[i], g["center"])
        assert res.center_flags[i] == cc.FLAG[g["class"]], name
        assert B.bits_hash(*nc.messages_of((res[i].bits(), res[i].msg_off, res[i].pauses))) == g["hash"], name
        if r[1] == 2:
            assert res.centers[i] is None and res.center_flags[i] == 0 and res[i].n_samples == 2 and res.qad(i).shape[0] == 2
    # the neighbours of the constant envelope and of the refused capture are what they are alone: the clean capture first and last
    assert res.centers[0] == res.centers[6] and all(np.array_equal(x, y) for x, y in zip(got_of(res[0]), got_of(res[6])))
    assert len(res[2].bits()) > 0 and res[2].n_samples == len(caps[2])
    with pytest.raises(OverflowError):
        res.check()


def _raw_center(pipe, qad, total, starts, k, p, lead, scratch_bytes, cap_thr, cap_res, cap_tie, max_size=-1):
    """urhgpu_batch_center_dev on buffers this test owns, each larger than what the library is told and filled with a sentinel"""
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    dev = pipe.device
    fill = lambda nbytes: torch.full((nbytes,), BE.SENTINEL, dtype=torch.uint8, device=dev)      # noqa: E731
    rb = C.sizeof(_lib.BatchCenterResult)
    d_qad = torch.from_numpy(qad).to(dev)
    d_start = torch.from_numpy(np.asarray(starts, np.int64)).to(dev)
    d_scratch, d_thr, d_res, d_tie = fill(2 * lead + scratch_bytes + 256), fill(2 * lead + 4 * cap_thr), fill(2 * lead + rb * cap_res), fill(2 * lead + 4 * cap_tie)
    cp = p.to_c(np.float32)
    pipe.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    st = lib.urhgpu_batch_center_dev(pipe.ctx.handle, C.c_void_p(d_qad.data_ptr()), total, C.c_void_p(d_start.data_ptr()), k, C.byref(cp), max_size, None,
                                     C.c_void_p(d_scratch.data_ptr() + lead), scratch_bytes, C.c_void_p(d_thr.data_ptr() + lead), cap_thr,
                                     C.c_void_p(d_res.data_ptr() + lead), cap_res, C.c_void_p(d_tie.data_ptr() + lead), cap_tie)
    torch.cuda.synchronize(dev)
    return st, [t.cpu().numpy() for t in (d_scratch, d_thr, d_res, d_tie)]


def test_c_abi_guards(pipe, oracle):
    """Capacities one element too small: scratch, thresholds and result blocks are refused before anything is launched -- nothing is
    written at all --; a tie pool one count too small drops that capture's counts (n_counts = 0) and nothing is written behind it.
    Malformed starts: the refused capture has no center, its neighbours are exact, nothing is written outside what the library was told."""
    from urh_amd import _lib, batch
    p = B.gain_params("FSK")
    tied = _by_class(oracle, "FSK", ("tie",))[:2]
    okc = _by_class(oracle, "FSK", ("ok",))[:1]
    refs = [B.reference(oracle, iq, p, None, True, key=("guard", i)) for i, iq in enumerate(tied + okc)]
    qads = [r[2][1] for r in refs]
    k, lead = 3, 1 << 12
    cat = np.concatenate(qads + [np.full(64, 9.0, np.float32)])            # (64 samples nobody owns behind the captures)
    starts = np.concatenate([[0], np.cumsum([len(q) for q in qads])]).astype(np.int64)
    total = int(starts[-1])
    max_bins = int(_lib.load().urhgpu_center_hist_cap(pipe.ctx.handle))
    need, _, _ = batch.batch_center_plan(np.diff(starts), total, max_bins)
    rb = C.sizeof(_lib.BatchCenterResult)
    hists = [cc.histogram(q, None)[0] for q in qads]
    nb = [len(h) for h in hists]
    untouched = lambda a: (a == BE.SENTINEL).all()                                  # noqa: E731

    def run(scratch=need, thr=k, res=k + 1, tie=nb[0] + nb[1], st_=starts):
        return _raw_center(pipe, cat, total, st_, k, p, lead, scratch, thr, res, tie)
    for kw in ({"scratch": need - 1}, {"thr": k - 1}, {"res": k}):
        st, bufs = run(**kw)
        assert st == _lib.ERR_CAPACITY and all(untouched(b) for b in bufs), kw
    st, (scratch, thr, res, tie) = run()
    assert st == 0
    assert untouched(scratch[:lead]) and untouched(scratch[lead + need:]) and untouched(thr[:lead]) and untouched(thr[lead + 4 * k:])
    assert untouched(res[:lead]) and untouched(res[lead + rb * (k + 1):]) and untouched(tie[:lead]) and untouched(tie[lead + 4 * (nb[0] + nb[1]):])
    blocks = (_lib.BatchCenterResult * (k + 1)).from_buffer_copy(res[lead:lead + rb * (k + 1)].tobytes())
    assert [int(b.r.flag) for b in blocks[:k]] == [3, 3, 1] and blocks[k].counts_off == nb[0] + nb[1]
    counts = tie[lead:lead + 4 * (nb[0] + nb[1])].view(np.uint32)
    for i in (0, 1):
        assert blocks[i].r.n_counts == nb[i] and np.array_equal(counts[blocks[i].counts_off:blocks[i].counts_off + nb[i]], hists[i]), i
    assert blocks[2].r.center == refs[2][2][0]
    want_thr = batch.center_thresholds(p, [None, None, refs[2][2][0]]).reshape(-1)
    assert np.array_equal(thr[lead:lead + 4 * k].view(np.float32), want_thr)
    # the pool one count too small: one of the two histograms does not fit
    st, (_, _, res, tie) = run(tie=nb[0] + nb[1] - 1)
    assert st == 0 and untouched(tie[:lead]) and untouched(tie[lead + 4 * (nb[0] + nb[1] - 1):])
    blocks = (_lib.BatchCenterResult * (k + 1)).from_buffer_copy(res[lead:lead + rb * (k + 1)].tobytes())
    assert sorted(int(blocks[i].r.n_counts) for i in (0, 1)) in ([0, nb[0]], [0, nb[1]]) and blocks[0].r.flag == blocks[1].r.flag == 3
    # malformed starts: capture 2 ends beyond the buffer the library was told (the allocation holds 64 more samples)
    bad = starts.copy()
    bad[2] = starts[2]
    bad[3] = total + 40
    st, (scratch, thr, res, tie) = run(st_=bad)
    assert st == 0 and untouched(scratch[:lead]) and untouched(scratch[lead + need:]) and untouched(res[lead + rb * (k + 1):])
    blocks = (_lib.BatchCenterResult * (k + 1)).from_buffer_copy(res[lead:lead + rb * (k + 1)].tobytes())
    assert blocks[2].r.flag == 0 and blocks[2].r.kept == 0 and blocks[2].r.n_bins == 0
    assert blocks[0].r.flag == blocks[1].r.flag == 3 and blocks[0].r.n_counts == nb[0] and blocks[1].r.n_counts == nb[1]
    neg = starts.copy()
    neg[0] = -5
    st, (_, _, res, _) = run(st_=neg)
    blocks = (_lib.BatchCenterResult * (k + 1)).from_buffer_copy(res[lead:lead + rb * (k + 1)].tobytes())
    assert st == 0 and blocks[0].r.flag == 0 and blocks[0].r.kept == 0 and blocks[1].r.flag == 3 and blocks[2].r.center == refs[2][2][0]
