"""DevicePipeline.iq_to_bits_batch_auto and detect_noise_levels (urh_amd/batch/, urh_amd/csrc/batch_auto.hip; include/urhgpu.h "a batch of
captures: automatic noise threshold per capture") against the oracle: every capture of a batch comes back with the threshold that
detect_noise_level gives for it alone and with the pulse table, bits, offsets, pauses and demodulated signal of the reference gated with
THAT threshold, whatever lies beside it in the buffer.  Every result is compared with the oracle (noise_cases.oracle_threshold /
noise_cases.reference), never with another HIP path alone.  The demodulated signal is compared by bits (edge_inputs.same_bits: where both
sides hold a NaN, its payload is not compared -- the capture with a NaN sample)."""
import ctypes as C

import numpy as np
import pytest

import batch_auto_cases as bc
import batch_edge_cases as B
import edge_inputs as E
import noise_cases as nc

pytestmark = pytest.mark.gpu

_want = {}


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def want(oracle, iq, p, key):
    """(threshold or the exception, flag, qad, pulse table, flat) of the reference for a capture: computed once per key, left unchanged"""
    key = (key, p.modulation_type, p.bits_per_symbol)
    if key not in _want:
        thr, flag = nc.oracle_threshold(oracle, iq)
        if flag == 1:
            qad, pp, flat = nc.reference(oracle, iq, p, thr)
        elif flag == 2:                                    # Signal.py:474-484: nothing is demodulated, zeros(2) are sliced
            qad = np.zeros(2, np.float32)
            pp, flat = nc.slice_qad(oracle, qad, p)
        else:
            qad = pp = flat = None
        _want[key] = (thr, flag, qad, None if pp is None else np.asarray(pp).reshape(-1, 2), flat)
    return _want[key]


def same(h, w, qad=None, tag=None):
    _, _, wq, pp, flat = w
    assert h.truncated == 0 and h.rows_needed == len(pp), (tag, h.truncated, h.rows_needed, len(pp))
    assert np.array_equal(h.ppseq(), pp), tag
    assert np.array_equal(h.bits(), flat[0]) and np.array_equal(h.msg_off, flat[1]) and np.array_equal(h.pauses, flat[2]), tag
    if qad is not None:
        got = qad.cpu().numpy()                             # bit for bit; a NaN (the capture with a NaN sample) equals a NaN, as in tests/edge_inputs.py
        assert got.shape == wq.shape and E.same_bits(got, wq).all(), tag


def check_all(res, oracle, caps, p, key, want_qad=True):
    """every capture of `res` against the oracle; returns the number of non-zero thresholds"""
    assert len(res) == len(caps) and res.truncated == []
    nonzero = 0
    for i, iq in enumerate(caps):
        w = want(oracle, iq, p, (key, i))
        assert res.noise_flags[i] == w[1] == 1, (key, i, len(iq))
        assert res.noise[i].hex() == float(w[0]).hex(), (key, i, len(iq), res.noise[i], w[0])
        assert res[i].n_samples == len(iq) and res[i].seq == i
        same(res[i], w, res.qad(i) if want_qad else None, (key, i, len(iq)))
        nonzero += res.noise[i] != 0.0
    return nonzero


SWEEP_RUNS = [(dt, "FSK", 1) for dt in nc.DTYPES5] + [(dt, mod, bps) for dt in (np.float32, np.int16) for mod, bps in (("ASK", 1), ("FSK", 2))]


@pytest.mark.parametrize("dtype,mod,bps", SWEEP_RUNS, ids=lambda v: v if isinstance(v, (str, int)) else np.dtype(v).name)
def test_size_sweep(pipe, oracle, dtype, mod, bps):
    name = np.dtype(dtype).name
    caps = bc.sweep(dtype)
    p = nc.params(mod, bps, write_pos=False)
    res = pipe.iq_to_bits_batch_auto(caps, p, want_qad=True, cap_rows="bound")
    assert check_all(res, oracle, caps, p, ("sweep", name)) == bc.SWEEP_NONZERO[name]
    golden = bc.load_golden()["sweep"][name]                # the real reference's thresholds
    assert [x.hex() for x in res.noise] == golden


def _flag_batch(pipe, oracle, named, p, key, expect_flags):
    caps = [np.ascontiguousarray(c) for _, c in named]
    res = pipe.iq_to_bits_batch_auto(caps, p, want_qad=True, cap_rows="bound")
    assert res.noise_flags == expect_flags
    for i, (name, iq) in enumerate(named):
        w = want(oracle, iq, p, (key, name))
        assert w[1] == expect_flags[i], name
        if w[1] == 0:
            assert isinstance(w[0], OverflowError) and np.isinf(res.noise[i])
            with pytest.raises(OverflowError):
                res[i]
            continue
        assert res.noise[i].hex() == float(w[0]).hex(), name
        same(res[i], w, res.qad(i), name)
        assert res[i].n_samples == (2 if w[1] == 2 else len(iq)), name
        if w[1] == 2:
            assert len(w[2]) == 2 and res.qad(i).shape[0] == 2
    return res


def test_flags_float32(pipe, oracle):
    p = nc.params("FSK", 1, write_pos=False)
    named = bc.flag_captures_f32()
    res = _flag_batch(pipe, oracle, named, p, "flags-f32", [1, 1, 1, 1, 0, 2, 1])
    assert res.noise[:4] == [res.noise[6], 0.0, 0.0, 0.0] and res.noise[0] > 0 and res.noise[5] == 4.831
    assert np.array_equal(res[0].ppseq(), res[6].ppseq()) and np.array_equal(res[0].bits(), res[6].bits()) and len(res[0].bits()) > 0
    # the capture where the reference raises: at [k], at iteration and in check(); every other capture is handed out
    handed = []
    with pytest.raises(OverflowError):
        for h in res:
            handed.append(h)
    assert len(handed) == 4
    with pytest.raises(OverflowError):
        res.check()
    # the threshold of the first launch alone raises for that batch too, and gives the same values without that capture
    with pytest.raises(OverflowError):
        pipe.detect_noise_levels([c for _, c in named])
    rest = [c for n, c in named if n != "inf"]
    assert pipe.detect_noise_levels(rest) == [x for i, x in enumerate(res.noise) if i != 4]


def test_flags_int8(pipe, oracle):
    p = nc.params("FSK", 1, write_pos=False)
    res = _flag_batch(pipe, oracle, bc.flag_captures_i8(), p, "flags-i8", [1, 2, 1])
    assert res.noise[1] == 181.0194 and res.noise[0] == res.noise[2] > 0
    res.check()


def test_neighbours_on_the_device(pipe, oracle):
    """the captures already back to back on the device, (iq_cat, starts): odd first samples, samples nobody owns in front and behind, loud
    captures of odd lengths between the others -- one of them directly in front of the quietest -- : the list form's results"""
    import torch
    p = nc.params("FSK", 1, write_pos=False)
    sweep = bc.sweep(np.float32)
    pick = [sweep[i] for i in (7, 13, 17, 20, 9)]            # 101, 801, 12 801, 65 537 and 200 samples: gains over 20 dB apart
    rng = np.random.default_rng(5)
    loud = lambda n: (3.0 * rng.standard_normal((n, 2))).astype(np.float32)      # noqa: E731
    caps = []
    for c in pick:
        caps += [loud(int(rng.integers(1, 40)) * 2 + 1), c]
    parts = [loud(7)] + caps + [loud(33)]
    cat = np.concatenate(parts)
    starts = 7 + np.concatenate([[0], np.cumsum([len(c) for c in caps])])
    assert starts[0] % 2 == 1 and any(s % 2 == 1 for s in starts[1:])
    res = pipe.iq_to_bits_batch_auto((torch.from_numpy(cat).to(pipe.device), starts), p, want_qad=True, cap_rows="bound")
    noise = list(res.noise)
    for j, c in enumerate(pick):                             # (a result's views are valid until the pipeline's next batch: looked at first)
        i = 2 * j + 1
        w = want(oracle, c, p, ("neighbours", j))
        assert res.noise_flags[i] == 1 and noise[i].hex() == float(w[0]).hex()
        same(res[i], w, res.qad(i), ("neighbours", j))
    alone = pipe.iq_to_bits_batch_auto(pick, p, want_qad=True, cap_rows="bound")
    for j, c in enumerate(pick):
        w = want(oracle, c, p, ("neighbours", j))
        assert alone.noise[j] == noise[2 * j + 1] and alone.noise_flags[j] == 1
        same(alone[j], w, alone.qad(j), ("alone", j))
    assert len(set(alone.noise)) > 1                        # (no single threshold serves them)


def test_each_capture_equals_the_pass_that_detects_its_own_threshold(pipe, oracle):
    import torch
    p = nc.params("FSK", 1, write_pos=False)
    sweep = bc.sweep(np.float32)
    idx = (7, 13, 17, 19)
    caps = [sweep[i] for i in idx]
    res = pipe.iq_to_bits_batch_auto(caps, p, cap_rows="bound")
    for j, c in enumerate(caps):
        w = want(oracle, c, p, (("sweep", "float32"), idx[j]))
        one = pipe.iq_to_bits(torch.from_numpy(np.array(c)).to(pipe.device), p, auto_noise=True, cap_rows=len(c) // (p.tolerance + 1) + 2)
        assert one.noise_flag == res.noise_flags[j] == 1 and one.noise_threshold == res.noise[j] == float(w[0])
        h = one.host(pool={})
        assert np.array_equal(h.ppseq(), res[j].ppseq()) and np.array_equal(h.bits(), res[j].bits()) and np.array_equal(h.msg_off, res[j].msg_off)
        same(res[j], w, None, j)


def test_launches_and_copies_do_not_depend_on_the_number_of_captures(pipe, oracle):
    from urh_amd import batch
    p = nc.params("FSK", 1, write_pos=False)
    rng = np.random.default_rng(9)
    big = nc.capture(7300, 800_000, sigma=0.01, amp=0.5)
    lengths = rng.integers(0, 300, 5000)
    at = np.concatenate([[0], np.cumsum(lengths)])
    many = [big[a:b] for a, b in zip(at[:-1], at[1:])]
    for caps in (bc.sweep(np.float32)[9:12], many):
        before = batch.launch_counts(pipe)
        res = pipe.iq_to_bits_batch_auto(caps, p)
        after = batch.launch_counts(pipe)
        assert (after[0] - before[0], after[1] - before[1]) == (4, 3), len(caps)
        before = after
        levels = pipe.detect_noise_levels(caps)
        after = batch.launch_counts(pipe)
        assert (after[0] - before[0], after[1] - before[1]) == (1, 1), len(caps)
        assert levels == res.noise and len(levels) == len(caps)
        for i in range(0, len(caps), max(1, len(caps) // 60)):
            thr, flag = nc.oracle_threshold(oracle, np.ascontiguousarray(caps[i]))
            assert flag == res.noise_flags[i] == 1 and float(thr).hex() == levels[i].hex(), (i, len(caps[i]))
    assert sum(x != 0.0 for x in levels) > 100


def test_routing_by_long_from(pipe, oracle):
    p = nc.params("FSK", 1, write_pos=False)
    caps = [nc.capture(7400 + i, n, sigma=s, amp=a) for i, (n, (s, a)) in enumerate(zip((4999, 5000, 900, 5001, 12_801), nc.STREAM_GAINS))]
    batch = pipe.iq_to_bits_batch_auto(caps, p, want_qad=True, cap_rows="bound", long_from=2 ** 31 - 1)
    noise, flags = list(batch.noise), list(batch.noise_flags)
    assert flags == [1] * 5 and all(x > 0 for x in noise)
    ws = [want(oracle, c, p, ("routing", i)) for i, c in enumerate(caps)]
    for i, w in enumerate(ws):
        assert noise[i].hex() == float(w[0]).hex()
        same(batch[i], w, batch.qad(i), ("batch", i))
    routed = pipe.iq_to_bits_batch_auto(caps, p, want_qad=True, cap_rows="bound", long_from=5000)      # (the next batch: the views above are gone)
    assert routed.noise == noise and routed.noise_flags == flags
    for i, w in enumerate(ws):
        assert routed[i].seq == i and routed[i].n_samples == len(caps[i])
        same(routed[i], w, routed.qad(i), ("routed", i))
    # auto_noise=False is the plain batch
    plain = pipe.iq_to_bits_batch_auto(caps[:2], p, auto_noise=False, cap_rows="bound")
    assert plain.noise is None and plain.noise_flags is None and len(plain) == 2


def test_truncation_and_retry(pipe, oracle):
    p = nc.params("FSK", 1, write_pos=False)
    sweep = bc.sweep(np.float32)
    idx = (13, 17, 9, 19)
    caps = [sweep[i] for i in idx]
    ws = [want(oracle, c, p, (("sweep", "float32"), i)) for i, c in zip(idx, caps)]
    res = pipe.iq_to_bits_batch_auto(caps, p, want_qad=True, cap_rows=2)
    short = [j for j, w in enumerate(ws) if len(w[3]) > 2]
    assert res.truncated == short and len(short) >= 2
    for j, w in enumerate(ws):
        assert res.noise[j].hex() == float(w[0]).hex() and res[j].rows_needed == len(w[3])            # exact whatever fitted
        if j in short:
            assert res[j].truncated & 1 and np.array_equal(res[j].ppseq(), w[3][:2])
        else:
            same(res[j], w, res.qad(j), j)
    k = short[0]
    before = {j: (res[j].ppseq().copy(), res[j].bits().copy()) for j in range(len(caps)) if j != k}
    again = res.retry(k)
    same(again, ws[k], res.qad(k), ("retry", k))
    assert res[k] is again and k not in res.truncated
    for j, (pp, bits) in before.items():                                                        # the neighbours' views are untouched
        assert np.array_equal(res[j].ppseq(), pp) and np.array_equal(res[j].bits(), bits)


GUARD_CASES = ("end_beyond_total", "start_above_end", "negative_start")


@pytest.mark.parametrize("case", GUARD_CASES)
def test_c_abi_guards(pipe, oracle, case):
    """urhgpu_iq_to_bits_batch_auto_dev on buffers this test owns, every one larger than what the library is told and filled with a sentinel;
    every malformed value still points inside an allocation.  A capture whose start or end is refused is not read: its block says flag 1,
    noise 0, its counts say truncated = 8; nothing is written outside what the library was told, and the neighbours are exact."""
    import torch
    from urh_amd import _lib, batch
    from urh_amd.pipeline import HostBits
    lib = _lib.load()
    p = nc.params("FSK", 1, write_pos=False)
    sweep = bc.sweep(np.float32)
    caps = [sweep[13], sweep[9], sweep[14]]                  # 801, 200 and 900 samples
    k, lead, iq_lead = 3, 1 << 16, 64
    iq = np.concatenate(caps)
    total = len(iq)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in caps])]).astype(np.int64)
    bad = {"end_beyond_total": 2, "start_above_end": 1, "negative_start": 0}[case]
    if case == "end_beyond_total":
        starts[3] = total + 40                               # (the allocation holds 64 more samples)
    elif case == "start_above_end":
        starts[1] = starts[2] + 7                            # capture 0 grows over capture 1's samples and 7 of capture 2's
    else:
        starts[0] = -5                                       # (64 samples lie in front of d_iq)
    valid = [i for i in range(k) if i != bad]
    seen = {i: np.ascontiguousarray(iq[int(starts[i]):int(starts[i + 1])]) for i in valid}
    # the plan for what the pass will see: the valid captures' lengths, nothing for the refused one
    lengths = np.array([len(seen[i]) if i in seen else 0 for i in range(k)], np.int64)
    cp = p.to_c(np.float32)
    cp.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch.batch_plan(lengths, cp, "bound")
    sizes = [B.region_bytes(int(n), int(r), p.samples_per_symbol, p.bits_per_symbol) for n, r in zip(lengths, plan[k:2 * k])]
    dev = pipe.device
    pad = np.zeros((iq_lead, 2), np.float32)
    d_iq = torch.from_numpy(np.concatenate([pad, iq, pad])).to(dev)
    d_meta = torch.from_numpy(np.concatenate([starts, plan])).to(dev)
    fill = lambda nbytes: torch.full((nbytes,), B.SENTINEL, dtype=torch.uint8, device=dev)      # noqa: E731
    d_work, d_blob, d_qad, d_noise = fill(2 * lead + work_bytes), fill(2 * lead + blob_cap), fill(4 * (total + 2 * iq_lead)), fill(2 * lead + 64 * k)
    d_counts = torch.full((8 * k,), -1, dtype=torch.int64, device=dev)
    d_dir = torch.full((k + 1,), -1, dtype=torch.int64, device=dev)
    pipe.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.urhgpu_iq_to_bits_batch_auto_dev(
        pipe.ctx.handle, C.c_void_p(d_iq.data_ptr() + 8 * iq_lead), total, C.c_void_p(d_meta.data_ptr()), C.c_void_p(d_meta.data_ptr() + 8 * (k + 1)), k,
        C.byref(cp), C.c_void_p(d_qad.data_ptr() + 4 * iq_lead), C.c_void_p(d_work.data_ptr() + lead), work_bytes, C.c_void_p(d_counts.data_ptr()),
        C.c_void_p(d_dir.data_ptr()), C.c_void_p(d_blob.data_ptr() + lead), blob_cap, C.c_void_p(d_noise.data_ptr() + lead)))
    torch.cuda.synchronize(dev)
    work, blob, qad, noise = (t.cpu().numpy() for t in (d_work, d_blob, d_qad, d_noise))
    counts, dirs = d_counts.cpu().numpy().reshape(k, 8), d_dir.cpu().numpy()
    # the result blocks: 64 k bytes and nothing around them
    assert (noise[:lead] == B.SENTINEL).all() and (noise[lead + 64 * k:] == B.SENTINEL).all()
    blocks = (_lib.NoiseResult * k).from_buffer_copy(noise[lead:lead + 64 * k].tobytes())
    assert blocks[bad].flag == 1 and blocks[bad].noise == 0.0 and blocks[bad].n_chunks == 0 and blocks[bad].noise_sqrd == 0.0
    assert counts[bad][4] == 8 and counts[bad][3] == 0 and counts[bad][0] == 0
    host = np.ascontiguousarray(blob[lead:])
    q = qad.view(np.float32)
    for i in valid:                                          # the neighbours are exact
        w = want(oracle, seen[i], p, ("guards", case, i))
        assert blocks[i].flag == w[1] == 1 and float(blocks[i].noise).hex() == float(w[0]).hex(), (case, i)
        h = HostBits.from_blob(host.ctypes.data + int(dirs[i]), p, seq=i, n_samples=len(seen[i]))
        same(h, w, None, (case, i))
        if case != "start_above_end":                        # (there captures 0 and 2 overlap and both write the shared samples' values)
            got = q[iq_lead + int(starts[i]):iq_lead + int(starts[i + 1])]
            assert np.array_equal(got.view(np.uint32), w[2].view(np.uint32)), (case, i)
    assert any(blocks[i].noise > 0 for i in valid)
    # nothing outside what the library was told
    sent32 = np.uint32(B.SENTINEL * 0x01010101)
    wrote = np.zeros(len(q), bool)
    for i in valid:
        wrote[iq_lead + int(starts[i]):iq_lead + int(starts[i + 1])] = True
    assert (qad.view(np.uint32)[~wrote] == sent32).all(), case
    owned = np.zeros(len(work), bool)
    for i in valid:
        owned[lead + int(plan[i]):lead + int(plan[i]) + sizes[i]] = True
    assert (work[~owned] == B.SENTINEL).all(), case
    used = int(dirs[k])
    assert 0 < used <= blob_cap and (blob[:lead] == B.SENTINEL).all() and (blob[lead + used:] == B.SENTINEL).all()
