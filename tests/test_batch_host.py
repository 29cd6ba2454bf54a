"""The host side of a batch of captures (urh_amd/batch/, urhgpu_batch_plan; include/urhgpu.h "a batch of captures"): sizing, launch
order, routing, the result sequence over blobs built here with numpy from oracle results, the option errors, and the code objects'
metadata of the batch kernels.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import synth_fsk


def _cp(mod="FSK", bps=1, tol=5, sps=100, dtype=np.float32):
    from urh_amd.pipeline import DemodParams
    p = DemodParams(mod, bps, 0.0, 0.0, 1.0, tol, sps, 0.1, 8, False)
    return p, p.to_c(np.dtype(dtype))


def _region_bytes(n, rows, sps, bps):
    """a capture's region of the work buffer as include/urhgpu.h describes it: int32 {length, state} rows, one byte per bit, offsets, pauses"""
    up = lambda x: (x + 15) & ~15          # noqa: E731
    msg = rows // 2 + 1
    bits = (n // sps + rows // 2 + 2) * bps
    return up(8 * rows) + up(bits) + up(8 * (msg + 1)) + up(8 * msg)


@pytest.mark.parametrize("tol,sps,bps", [(5, 100, 1), (0, 8, 3), (70, 10, 2)])
def test_plan_follows_the_formulas(tol, sps, bps):
    from urh_amd import batch
    p, cp = _cp("FSK", bps, tol, sps)
    rng = np.random.default_rng(tol + sps)
    for lengths in ([], [12345], [0], list(rng.integers(0, 40000, 200)) + [0, 0, 1, 2, 2 ** 31 - 1]):
        lengths = np.asarray(lengths, dtype=np.int64)
        k = len(lengths)
        for policy in (None, "bound", 777):
            plan, work, blob = batch.batch_plan(lengths, cp, policy)
            off, rows = plan[:k], plan[k:2 * k]
            bound = lengths // (tol + 1) + 2
            if policy is None:
                want = np.minimum(bound, np.maximum(64, 4 * (lengths // sps) + 64))
            elif policy == "bound":
                want = bound
            else:
                want = np.full(k, 777)
            assert np.array_equal(rows, want)
            # the regions: disjoint, in order, 16-byte aligned, each what the capture's capacities need
            sizes = np.array([_region_bytes(int(n), int(r), sps, bps) for n, r in zip(lengths, rows)], dtype=np.int64)
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)[:-1]]) if k else off)
            assert work == int(sizes.sum()) and not (off % 16).any()
            assert blob >= 128 * k and blob % 16 == 0
            if k == 0:
                assert work == 0 and blob == 0


def test_launch_order_is_a_permutation_longest_first():
    from urh_amd import batch
    _, cp = _cp()
    rng = np.random.default_rng(3)
    lengths = np.concatenate([rng.integers(0, 5000, 1000), [0, 0, 70001, 70001, 5]]).astype(np.int64)
    plan, _, _ = batch.batch_plan(lengths, cp)
    order = plan[2 * len(lengths):]
    assert sorted(order.tolist()) == list(range(len(lengths)))
    assert (np.diff(lengths[order]) <= 0).all()


def test_plan_rejects_what_a_batch_does_not_take():
    from urh_amd import _lib, batch
    for mod in ("PSK", "QAM"):
        _, cp = _cp(mod)
        with pytest.raises(_lib.UrhGpuError) as e:
            batch.batch_plan([100], cp)
        assert e.value.status == _lib.ERR_UNSUPPORTED
    _, cp = _cp()
    for bad in ([-1], [2 ** 31]):
        with pytest.raises(_lib.UrhGpuError) as e:
            batch.batch_plan(bad, cp)
        assert e.value.status == _lib.ERR_ARG
    assert batch.batch_step() in (64, 128)


def test_routing_by_long_from():
    from urh_amd import batch
    lengths = [0, 10, 49_999, 50_000, 70_001, 3]
    short, long_ = batch.route(lengths, 50_000)
    assert short.tolist() == [0, 1, 2, 5] and long_.tolist() == [3, 4]
    short, long_ = batch.route(lengths)
    assert short.tolist() == list(range(6)) and long_.tolist() == [] and batch.LONG_FROM_DEFAULT > 70_001
    short, long_ = batch.route([batch.LONG_FROM_DEFAULT - 1, batch.LONG_FROM_DEFAULT])
    assert short.tolist() == [0] and long_.tolist() == [1]


def _blob(pp, bits, msg_off, pauses, rows_needed=None, truncated=0):
    """a standard compact result blob (include/urhgpu.h) as the batch's pack kernel lays it out: flags 0, no positions"""
    from urh_amd import _lib
    up = lambda x: (x + 15) & ~15          # noqa: E731
    n_rows, n_msg, n_bits = len(pp), len(pauses), len(bits)
    o = 128
    off_pauses = o; o = up(o + 8 * n_msg)
    off_msg = o; o = up(o + 8 * (n_msg + 1))
    off_pos_off = o; o = up(o + 8 * (n_msg + 1))
    off_state = o; o = up(o + n_rows)
    off_bits = o; o = up(o + (n_bits + 7) // 8)
    off_len = o; o = up(o + 4 * n_rows)
    total = o
    b = np.zeros(total, np.uint8)
    b[:128].view(np.int64)[:] = [_lib.BLOB_MAGIC, n_rows, n_msg, n_bits, 0, len(pp) if rows_needed is None else rows_needed, total, 0, off_pauses,
                                 off_msg, off_pos_off, off_state, off_bits, off_len, total, truncated]
    b[off_pauses:off_pauses + 8 * n_msg].view(np.int64)[:] = pauses
    b[off_msg:off_msg + 8 * (n_msg + 1)].view(np.int64)[:] = msg_off
    b[off_state:off_state + n_rows].view(np.int8)[:] = pp[:, 0]
    packed = np.packbits(bits)
    b[off_bits:off_bits + len(packed)] = packed
    b[off_len:off_len + 4 * n_rows].view(np.int32)[:] = pp[:, 1]
    return b


def test_batch_bits_over_blobs_built_from_oracle_results(oracle):
    from urh_amd import _lib
    from urh_amd.batch import BatchBits
    from urh_amd.pipeline import DemodParams, HostBits
    p = DemodParams("FSK", 1, 0.05, 0.0, 1.0, 5, 50, 0.1, 4, False)
    caps = [synth_fsk(n, sps=50, seed=n, noise=0.02, pause_every=2500, pause_len=pl) for n, pl in ((9000, 150), (0, 0), (3, 0), (20001, 320), (5000, 260))]
    want, blobs = [], []
    for iq in caps:
        qad = oracle.afp_demod(iq, 0.05, "FSK", 2)
        pp = oracle.grab_pulse_lens(qad, 0.0, 5, "FSK", 50, 1, 1.0).reshape(-1, 2)
        flat = oracle.ppseq_to_bits_flat(pp, 50, 1, True, 4)
        want.append((pp, flat))
        blobs.append(_blob(pp, flat[0], flat[1], flat[2]))
    # the last capture once more, as a truncated entry: half its rows stored, the need reported
    pp, flat = want[-1]
    blobs.append(_blob(pp[:len(pp) // 2], flat[0][:8], np.array([0]), np.zeros(0, np.int64), rows_needed=len(pp), truncated=1))
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blobs])])
    store = np.concatenate(blobs)
    assert not (offs % 16).any()
    items = [HostBits.from_blob(store.ctypes.data + int(offs[i]), p, seq=i, n_samples=len(c)) for i, c in enumerate(caps + [caps[-1]])]
    res = BatchBits(items, p, [len(c) for c in caps] + [len(caps[-1])])
    assert len(res) == 6 and [h.seq for h in res] == list(range(6)) and res[-1] is items[-1] and len(res[1:3]) == 2
    assert any(len(w[1][2]) > 1 for w in want)                 # (some capture holds more than one message)
    for h, (pp, flat) in zip(res, want):
        assert not h.truncated and h.check() is h
        assert np.array_equal(h.ppseq(), pp)
        got = h.flat()
        for a, b in zip(got, flat):                            # bits, msg_off, pauses, positions DERIVED from the rows, their offsets
            assert np.array_equal(a, b)
        assert np.array_equal(h.bit_sample_pos(), flat[3]) and np.array_equal(h.pos_offsets(), flat[4])
    assert res.truncated == [5] and res[5].rows_needed == len(want[-1][0])
    with pytest.raises(_lib.UrhGpuError):
        res[5].check()
    with pytest.raises(_lib.UrhGpuError):
        res.check()
    with pytest.raises(ValueError):
        res.qad(0)


def test_what_a_batch_does_not_do_raises_with_a_sentence():
    from urh_amd.batch import check_batch_options
    from urh_amd.pipeline import DemodParams
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
    check_batch_options(p)
    check_batch_options(p, auto_center=False, msg_records=False)
    for name in ("auto_center", "auto_noise", "msg_records", "dc_correction"):
        with pytest.raises(ValueError, match="call iq_to_bits"):
            check_batch_options(p, **{name: True})
    for mod in ("PSK", "QAM"):
        with pytest.raises(ValueError, match="CaptureStream"):
            check_batch_options(DemodParams(mod, 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False))
    with pytest.raises(TypeError):
        check_batch_options(p, no_such_option=1)
    # the method is there and checks before it touches a device
    from urh_amd.pipeline import DevicePipeline
    assert callable(DevicePipeline.iq_to_bits_batch)


@pytest.fixture(scope="module")
def batch_asm(tmp_path_factory):
    """batch.hip compiled to gfx950 assembly (no GPU needed), as tests/test_sniffer_host.py does for chunk_stats.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch") / "batch.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_batch_kernels_have_no_spills_and_no_scratch(batch_asm):
    """the code object's metadata of every k_batch_* kernel: no spilled vector or scalar registers, no private segment"""
    kernels = re.findall(r"\.name:\s+(\S*k_batch_\S+)", batch_asm)
    assert len(kernels) == 22, kernels                       # five sample types x ASK / FSK x order 2 / any order, the scan, the pack
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", batch_asm)]
        assert len(values) == 22 and not any(values), (key, values)
    assert "scratch_" not in batch_asm


def test_batch_assembly_holds_no_fp32_fma(batch_asm):
    """no v_fma_f32 / v_fmac_f32 / v_mac_f32 in batch.hip's assembly: nothing is contracted (-ffp-contract=off), and the quotients and square
    roots -- which the compiler would expand into fp32 FMAs -- are taken in fp64 and rounded once (batch.hip's URH_FDIV / URH_FSQRT: the same
    float for fp32 operands), so an fp32 FMA here could only be a multiply and an add of the source fused into one rounding"""
    assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", batch_asm)
    assert re.search(r"v_div_fixup_f64", batch_asm) and not re.search(r"v_div_fixup_f32", batch_asm)
