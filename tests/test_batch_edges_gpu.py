"""DevicePipeline.iq_to_bits_batch (urh_amd/csrc/batch.hip) on the inputs of tests/batch_edge_cases.py: edge VALUES through the batch's own
quotient and square root (fp64 rounded once to fp32), parameters no batch test had used, truncating and malformed plans, the second
fetch.  Every capture of every batch is compared with the oracle on that capture alone -- which tests/test_batch_edges_host.py pins to the
reference on the same inputs --: qad by bits (NaN equal to NaN), pulse table, bits, msg_off, pauses, positions and position offsets
exactly.  No tolerances.  Exactness runs use cap_rows="bound" and assert that nothing was truncated.

What each test is there to catch (a kernel with that change fails it):
  test_a1_*       lane 0's seam predecessor taken as 0 instead of the step before's lane 63; a neighbouring capture's sample read across
                  a capture's first / last sample
  test_a2_*, a4   batch.hip's URH_FDIV as a reciprocal multiply, URH_FSQRT / the conversions flushing denormals
  test_a3_*       `<=` of the noise gate as `<`, or taken on an exact instead of the rounded float32 sum
  test_a5_*       `<=` of classify as `<`
  test_b1_*       the initial state classify(0.0f, ...) replaced by the lowest state
  test_b2_*       states above 7 through the int8 store and the bit expansion's shifts
  test_b3_*       the symbol rounding 2 * rr > sps at sps 1 and odd sps
  test_b4_*       the expansion loop's second and third rounds (u += 64)
  test_b5_*       the directory scan at the ends of its 256 threads' stretches
  test_c1_*, c2   the `idx < cap_rows` guard of the row store removed (c2: the sentinel behind the region, inside the test's own memory)
  test_c3_*       a malformed entry followed into the buffers
  test_c4_*       the second fetch dropped or its buffer not grown"""

import numpy as np
import pytest

import batch_edge_cases as B
import edge_inputs as E

pytestmark = pytest.mark.gpu

_expected = {}


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


@pytest.fixture(scope="module")
def S():
    from urh_amd.batch import batch_step
    return batch_step()


def want(oracle, b, i):
    """the oracle on capture i of the batch alone: computed once per case, never changed"""
    key = (b.tag, i)
    if key not in _expected:
        _expected[key] = B.expected(oracle, b.caps[i][1], b)
    return _expected[key]


def same(h, ref, qad, what):
    wq, pp, flat = ref
    assert h.truncated == 0 and h.rows_needed == len(pp), (what, h.truncated, h.rows_needed, len(pp))
    if qad is not None:
        got = qad.cpu().numpy()
        ok = E.same_bits(got, wq)
        bad = np.nonzero(~ok)[0]
        assert got.shape == wq.shape and len(bad) == 0, (what, "qad", len(bad), bad[:6], got[bad[:6]], wq[bad[:6]])
    assert np.array_equal(h.ppseq(), pp), (what, "pulse table")
    assert np.array_equal(h.bits(), flat[0]) and np.array_equal(h.msg_off, flat[1]) and np.array_equal(h.pauses, flat[2]), (what, "bits")
    assert np.array_equal(h.bit_sample_pos(), flat[3]) and np.array_equal(h.pos_offsets(), flat[4]), (what, "positions")
    for k, (a, c) in enumerate(zip(h.flat(), flat)):
        assert np.array_equal(a, c), (what, ("bits", "msg_off", "pauses", "pos", "pos_off")[k])


def run_exact(pipe, oracle, b, want_qad=True):
    res = pipe.iq_to_bits_batch(b.arrays(), b.params(), want_qad=want_qad, cap_rows="bound")
    assert len(res) == len(b.caps) and res.truncated == []
    for i, (name, iq) in enumerate(b.caps):
        assert res[i].n_samples == len(iq) and res[i].seq == i
        same(res[i], want(oracle, b, i), res.qad(i) if want_qad else None, (b.tag, i, name))
    if b.twins:                                            # nothing carries over between wavefronts: the same capture, the same result
        i, j = b.twins
        assert np.array_equal(res[i].ppseq(), res[j].ppseq()) and np.array_equal(res[i].bits(), res[j].bits())
        if want_qad:
            assert np.array_equal(res.qad(i).cpu().numpy().view(np.uint32), res.qad(j).cpu().numpy().view(np.uint32))
    return res


# ---- A: values -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_a1_specials_at_the_step_seams(pipe, oracle, S, mod, bps):
    run_exact(pipe, oracle, B.a1_batch(mod, bps, S))


@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_a1_non_finite_samples_either_side_of_a_capture_boundary(pipe, oracle, S, mod):
    run_exact(pipe, oracle, B.a1_adjacent(mod, S))


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_a2_scaled_into_the_denormals_and_beyond_overflow(pipe, oracle, S, mod, bps):
    for k in B.SCALE_K:
        run_exact(pipe, oracle, B.a2_batch(mod, bps, k, S))


@pytest.mark.parametrize("mod", ["FSK", "ASK"])
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_a3_ties_on_the_noise_gate(pipe, oracle, S, mod, dtype):
    for bps in ((1, 2) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.int16)) else (1,)):
        for b in B.a3_batch(mod, dtype, bps, S):
            run_exact(pipe, oracle, b)


@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_a3_tie_at_threshold_zero(pipe, oracle, S, mod):
    b = B.a3_zero_threshold(mod, S)
    res = run_exact(pipe, oracle, b)
    assert (res.qad(1).cpu().numpy()[b.info["at"]] == oracle.noise_for_mod_type(mod)).all()


@pytest.mark.parametrize("mod", ["FSK", "ASK"])
@pytest.mark.parametrize("dtype", B.INT_DTYPES)
def test_a4_ends_of_the_integer_ranges(pipe, oracle, S, mod, dtype):
    for half in (False, True):
        run_exact(pipe, oracle, B.a4_batch(mod, dtype, half, S))


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_a5_samples_equal_to_a_threshold(pipe, oracle, S, dtype, bps):
    b = B.a5_batch(dtype, bps, S)
    res = run_exact(pipe, oracle, b)
    assert int((res.qad(1).cpu().numpy() == B.a5_threshold(dtype)).sum()) >= 100


# ---- B: parameters -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [0, 5])
def test_b1_initial_state_is_that_of_zero(pipe, oracle, tol):
    tables = []
    for bps, spacing, center in B.B1_CASES:
        res = run_exact(pipe, oracle, B.b1_batch(bps, spacing, center, tol))
        tables.append((bps, res[1].ppseq().tolist()))       # (the capture of two samples)
    one, two = [t for bps, t in tables if bps == 1], [t for bps, t in tables if bps == 2]
    assert one[0] != one[1] and len({str(t) for t in two}) == 4


@pytest.mark.parametrize("bps", [4, 5, 6, 7])
@pytest.mark.parametrize("mod", ["FSK", "ASK"])
def test_b2_sixteen_to_128_states(pipe, oracle, S, mod, bps):
    res = run_exact(pipe, oracle, B.b2_batch(mod, bps, S))
    assert int(res[0].ppseq()[:, 0].max()) == 2 ** bps - 1


@pytest.mark.parametrize("sps", [1, 3, 7])
def test_b3_small_and_odd_samples_per_symbol(pipe, oracle, sps):
    run_exact(pipe, oracle, B.b3_batch(sps))


@pytest.mark.parametrize("bps", [1, 3])
def test_b4_rows_of_more_than_64_symbols(pipe, oracle, bps):
    run_exact(pipe, oracle, B.b4_batch(bps))


@pytest.mark.parametrize("k", [255, 256, 257, 513])
def test_b5_captures_around_the_scans_256_threads(pipe, oracle, k):
    res = run_exact(pipe, oracle, B.b5_batch(k), want_qad=False)
    assert len(res) == k


# ---- C: guards and truncation ----------------------------------------------------------------------------------------------------------------
def assert_prefix(h, ref, cap, b, what):
    """a capture whose table has more rows than `cap`: the first cap rows, and _ppseq_to_bits over exactly those"""
    import urh_oracle
    _, pp, _ = ref
    assert h.truncated & 1 and not h.truncated & ~1, (what, h.truncated)
    assert h.rows_needed == len(pp) and h.n_rows == cap, (what, h.rows_needed, h.n_rows)
    assert np.array_equal(h.ppseq(), pp[:cap]), what
    flat = urh_oracle.ppseq_to_bits_flat(pp[:cap], b.sps, b.bps, True, b.pt)
    assert np.array_equal(h.bits(), flat[0]) and np.array_equal(h.msg_off, flat[1]) and np.array_equal(h.pauses, flat[2]), what


def test_c1_fixed_row_capacities(pipe, oracle):
    from urh_amd import _lib
    b = B.c1_batch()
    refs = [want(oracle, b, i) for i in range(3)]
    R = len(refs[1][1])
    assert 50 <= R <= 200 and [len(r[1]) for r in refs] == [1, R, 2]
    for cap in (0, 1, 2, R - 1, R, R + 1):
        res = pipe.iq_to_bits_batch(b.arrays(), b.params(), want_qad=True, cap_rows=cap)
        short = [i for i, r in enumerate(refs) if len(r[1]) > cap]
        assert res.truncated == short, (cap, res.truncated)
        assert (1 in short) == (cap < R)
        for i in range(3):
            if i in short:
                assert_prefix(res[i], refs[i], cap, b, (cap, i))
                with pytest.raises(_lib.UrhGpuError):
                    res[i].check()
                assert E.same_bits(res.qad(i).cpu().numpy(), refs[i][0]).all()        # (the demodulated signal does not depend on the rows)
            else:
                same(res[i], refs[i], res.qad(i), (cap, i))
        for i in short:                                    # once more alone with the rows it asked for; the others' views stay as they are
            again = res.retry(i)
            assert again is res[i]
            same(again, refs[i], res.qad(i), (cap, i, "retry"))
            for j in range(3):
                if j in short and j > i:
                    assert_prefix(res[j], refs[j], cap, b, (cap, j, "after the retry of", i))
                else:
                    same(res[j], refs[j], res.qad(j), (cap, j, "after the retry of", i))
        assert res.truncated == []


def _raw_setup(b, cap_rows, S):
    """(capture arrays, lengths, C parameters, the plan of cap_rows rows per capture, each capture's region bytes under that plan and under
    the "bound" policy)"""
    from urh_amd import batch
    caps = b.arrays()
    lengths = np.array([len(c) for c in caps], np.int64)
    cp = b.params().to_c(caps[0].dtype)
    cp.write_bit_sample_pos = 0
    plan, _, _ = batch.batch_plan(lengths, cp, cap_rows)
    k = len(caps)
    small = [B.region_bytes(int(n), int(r), b.sps, b.bps) for n, r in zip(lengths, plan[k:2 * k])]
    bound = [B.region_bytes(int(n), int(n) // (b.tol + 1) + 2, b.sps, b.bps) for n in lengths]
    return caps, lengths, cp, plan, small, bound


def _blob_view(run, i, p, n):
    from urh_amd.pipeline import HostBits
    host = np.ascontiguousarray(run.blob[run.lead:])
    h = HostBits.from_blob(host.ctypes.data + int(run.dir[i]), p, seq=i, n_samples=n)
    h._keep = host
    return h


def test_c2_nothing_is_written_outside_a_region(pipe, oracle, S):
    """a plan of 4 rows per capture, the regions moved apart by hand: behind every region a gap as large as the region the "bound" policy
    would give that capture, so that even a store without its guard lands in memory this test allocated, where the sentinel shows it"""
    b = B.c1_batch()
    b.caps = b.caps + [("other", B.b3_batch(3).caps[1][1])]
    caps, lengths, cp, plan, small, bound = _raw_setup(b, 4, S)
    k = len(caps)
    lead = max(bound) + 4096
    lead += -lead % 16
    off, at = [], 0                                        # (offsets from the pointer the library gets, which lies `lead` bytes inside the allocation)
    for i in range(k):
        off.append(at)                                     # region, gap, region, gap, ...
        at += small[i] + bound[i] + 64
        at += -at % 16
    work_bytes = at                                        # declared: up to the end of the last gap
    work_alloc = lead + work_bytes + lead                  # the same slack in front of the first region and behind the last gap
    plan = plan.copy()
    plan[:k] = off
    blob_cap = sum(B.blob_bytes(int(n) // (b.tol + 1) + 2, int(n), 8 * int(n)) for n in lengths) + 4096
    blob_cap += -blob_cap % 16
    iq = np.concatenate(caps)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    pad = np.zeros((64, 2), iq.dtype)
    run = B.run_raw(pipe.ctx, np.concatenate([pad, iq, pad]), 64, len(iq), starts, plan, k, cp, work_alloc, work_bytes, lead + blob_cap + lead, blob_cap, lead)
    refs = [B.expected(oracle, c, b) for c in caps]
    # the results: truncated to 4 rows where the table is longer, exact otherwise
    for i in range(k):
        h = _blob_view(run, i, b.params(), len(caps[i]))
        assert run.counts[i][3] == len(refs[i][1])
        if len(refs[i][1]) > 4:
            assert_prefix(h, refs[i], 4, b, i)
        else:
            same(h, refs[i], None, i)
    assert len(refs[1][1]) > 50                            # (a store without its guard would have had somewhere to go)
    # the work buffer: only the regions were written
    owned = np.zeros(len(run.work), bool)
    for i in range(k):
        owned[lead + off[i]:lead + off[i] + small[i]] = True
    outside = run.work[~owned]
    assert (outside == B.SENTINEL).all(), ("written outside the regions", int((outside != B.SENTINEL).sum()), np.nonzero(~owned & (run.work != B.SENTINEL))[0][:8] - lead)
    assert (run.work[owned] != B.SENTINEL).any()
    # the blob buffer: nothing in front, nothing beyond d_dir[k]
    used = int(run.dir[k])
    assert 0 < used <= blob_cap and (run.blob[:lead] == B.SENTINEL).all() and (run.blob[lead + used:] == B.SENTINEL).all()
    # the demodulated signal: the captures' samples and nothing else
    q = run.qad.view(np.uint32)
    sent = np.uint32(B.SENTINEL * 0x01010101)
    assert (q[:64] == sent).all() and (q[64 + len(iq):] == sent).all()
    assert E.same_bits(run.qad.view(np.float32)[64:64 + len(iq)], np.concatenate([r[0] for r in refs])).all()


C3_CASES = ("end_beyond_total", "start_above_end", "negative_start", "offset_not_16", "region_beyond_work", "negative_capacity")


@pytest.mark.parametrize("case", C3_CASES)
def test_c3_a_malformed_entry_is_refused_and_its_neighbours_are_exact(pipe, oracle, S, case):
    """truncated bit 3.  Every allocation is larger than what the library is told and every wrong value still points inside it.  A capture
    whose START or END is bad is not read at all: no rows needed, an empty blob, nothing in its qad slice.  One whose PLAN ENTRY alone is
    bad is still demodulated and counted -- its samples are valid --: qad slice and rows_needed are the oracle's, truncated bits 0 and 3
    are set, nothing is stored in the work buffer and its blob is empty."""
    from urh_amd import _lib
    b = B.b3_batch(3)
    b.caps = [b.caps[0], b.caps[1], ("third", b.caps[0][1][:500].copy())]
    caps, lengths, cp, plan, small, bound = _raw_setup(b, "bound", S)
    k = 3
    iq = np.concatenate(caps)
    total = len(iq)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lead = max(bound) + 4096
    lead += -lead % 16
    work_bytes = int(plan[k - 1]) + small[k - 1]
    bad, entry_only = {"end_beyond_total": 2, "start_above_end": 1, "negative_start": 0}.get(case, 1), case in C3_CASES[3:]
    plan = plan.copy()
    if case == "end_beyond_total":
        starts[3] = total + 40                             # (the allocation holds 64 more samples)
    elif case == "start_above_end":
        starts[1] = starts[2] + 7                          # capture 0 grows over capture 1's samples and 7 of capture 2's; its region must hold that
        n0 = int(starts[1])
        grow = B.region_bytes(n0, n0 // (b.tol + 1) + 2, b.sps, b.bps) - small[0]
        plan[k] = n0 // (b.tol + 1) + 2
        plan[1:k] += grow
        small[0] += grow
        work_bytes += grow
    elif case == "negative_start":
        starts[0] = -5                                     # (64 samples lie in front of d_iq)
    elif case == "offset_not_16":
        plan[1] += 8
    elif case == "region_beyond_work":
        plan[1] = work_bytes - 16                          # (the allocation goes on for `lead` bytes, more than the region)
    elif case == "negative_capacity":
        plan[k + 1] = -3
    blob_cap = sum(B.blob_bytes(int(n) + 2, int(n), 8 * int(n)) for n in (lengths + 64)) + 4096
    blob_cap += -blob_cap % 16
    pad = np.zeros((64, 2), iq.dtype)
    run = B.run_raw(pipe.ctx, np.concatenate([pad, iq, pad]), 64, total, starts, plan, k, cp, lead + work_bytes + lead, work_bytes, lead + blob_cap + lead,
                    blob_cap, lead)
    valid = [i for i in range(k) if i != bad]
    seen = {i: np.ascontiguousarray(iq[int(starts[i]):int(starts[i + 1])]) for i in valid}
    refs = {i: B.expected(oracle, seen[i], b) for i in valid}
    # (start_above_end: captures 0 and 2 overlap in [start[2], start[1]) and both write those samples' qad -- the same floats but at
    # start[2], capture 2's first sample, which has no predecessor there: either value)
    either = int(starts[2]) if case == "start_above_end" else -1
    for i in valid:                                        # the neighbours are exact
        same(_blob_view(run, i, b.params(), len(seen[i])), refs[i], None, (case, i))
        ok = E.same_bits(run.qad.view(np.float32)[64 + int(starts[i]):64 + int(starts[i + 1])], refs[i][0])
        if int(starts[i]) <= either < int(starts[i + 1]):
            ok[either - int(starts[i])] = True
        assert ok.all(), (case, i, np.nonzero(~ok)[0][:8])
    # the refused capture: bit 3, nothing stored, a well-formed empty blob
    cnt = run.counts[bad]
    assert cnt[4] & 8 and cnt[0] == 0 and cnt[1] == 0 and cnt[2] == 0, (case, cnt)
    at = lead + int(run.dir[bad])
    hdr = run.blob[at:at + 128].view(np.int64)
    assert hdr[0] == _lib.BLOB_MAGIC and hdr[1] == hdr[2] == hdr[3] == hdr[4] == 0 and hdr[15] == cnt[4] and hdr[6] == B.blob_bytes(0, 0, 0)
    assert int(run.dir[bad + 1] - run.dir[bad]) == B.blob_bytes(0, 0, 0)
    assert run.blob[at + hdr[9]:at + hdr[9] + 8].view(np.int64)[0] == 0                       # msg_off[0]
    h = _blob_view(run, bad, b.params(), 0)
    assert h.n_rows == 0 and h.n_msg == 0 and h.n_bits == 0 and len(h.bits()) == 0 and h.msg_off.tolist() == [0] and h.truncated & 8
    sent = np.uint32(B.SENTINEL * 0x01010101)
    q = run.qad.view(np.uint32)
    if entry_only:                                         # still demodulated and counted: what the header says of a bad plan entry
        ref = B.expected(oracle, caps[bad], b)
        assert cnt[3] == len(ref[1]) and cnt[4] == 9, (case, cnt)
        assert E.same_bits(run.qad.view(np.float32)[64 + int(starts[bad]):64 + int(starts[bad + 1])], ref[0]).all()
    else:                                                  # not read at all
        assert cnt[3] == 0 and cnt[4] == 8, (case, cnt)
    wrote = np.zeros(len(q), bool)
    for i in valid + ([bad] if entry_only else []):
        wrote[64 + int(starts[i]):64 + int(starts[i + 1])] = True
    assert (q[~wrote] == sent).all(), (case, "qad written outside the valid captures", np.nonzero(~wrote & (q != sent))[0][:8] - 64)
    # the sentinel is intact outside what the valid captures own
    owned = np.zeros(len(run.work), bool)
    for i in valid:
        owned[lead + int(plan[i]):lead + int(plan[i]) + small[i]] = True
    assert (run.work[~owned] == B.SENTINEL).all(), (case, np.nonzero(~owned & (run.work != B.SENTINEL))[0][:8] - lead)
    used = int(run.dir[k])
    assert (run.blob[:lead] == B.SENTINEL).all() and (run.blob[lead + used:] == B.SENTINEL).all()


def test_c4_blobs_beyond_the_first_host_buffer_take_a_second_fetch(oracle):
    from urh_amd import batch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    first = batch.FIRST_BLOB_BUFFER_BYTES
    assert first == 8 << 20
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 0, 8, 0.1, 8, False)
    noise = (0.3 * np.random.default_rng(41).standard_normal((60_000, 2))).astype(np.float32)
    qad = oracle.afp_demod(noise, 0.0, "FSK", 2)
    pp = np.asarray(oracle.grab_pulse_lens(qad, 0.0, 0, "FSK", 8, 1, 1.0)).reshape(-1, 2)
    flat = oracle.ppseq_to_bits_flat(pp, 8, 1, True, 8)
    one = B.blob_bytes(len(pp), len(flat[2]), len(flat[0]))
    # (the pinned buffer is made a quarter larger than asked for -- urh_amd/batch/staging.py::_pinned --: the first fetch is refused from 10 MiB on, so
    # the total is taken 35 % above the constant, which is "at least 10 %" as well)
    m = -(-(first + first // 4 + first // 10) // one) + 1
    total = m * one
    assert total >= 1.35 * first and m <= 100, (m, one, total)
    pipe = DevicePipeline(0)                               # fresh: its pinned blob buffer has not grown yet
    before = batch.launch_counts(pipe)
    res = pipe.iq_to_bits_batch([noise] * m, p, want_qad=False, cap_rows="bound")
    after = batch.launch_counts(pipe)
    # three launches; the directory, the directory again after the refused fetch, the blob (urhgpu_batch_fetch counts every copy it issues)
    assert (after[0] - before[0], after[1] - before[1]) == (3, 3)
    assert pipe._pinned["batch_blob"].numel() >= total > first + first // 4
    assert len(res) == m and res.truncated == []
    assert sum(h.blob_bytes for h in res) == total
    for i in range(m):
        same(res[i], (qad, pp, flat), None, i)
