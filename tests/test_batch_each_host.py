"""A batch with parameters per capture, what needs no GPU (urh_amd/batch/each.py; include/urhgpu.h "a batch of captures: parameters per
capture"): urhgpu_batch_plan_each's arithmetic, the per-capture table, every refusal of check_batch_each_options, params_from_estimates, and
the new kernels' code object (no spills, no scratch, no fp32 FMA)."""
import json
import os
import re
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from conftest import ROOT


def dp(mod="FSK", bps=1, tol=5, sps=100, pt=8, noise=0.0, center=0.0, spacing=1.0):
    from urh_amd.pipeline import DemodParams
    return DemodParams(mod, bps, noise, center, spacing, tol, sps, 0.1, pt, False)


def _region_bytes(n, rows, sps, bps):
    """a capture's region of the work buffer as include/urhgpu.h describes it: int32 {length, state} rows, one byte per bit, offsets, pauses"""
    up = lambda x: (x + 15) & ~15          # noqa: E731
    msg = rows // 2 + 1
    bits = (n // sps + rows // 2 + 2) * bps
    return up(8 * rows) + up(bits) + up(8 * (msg + 1)) + up(8 * msg)


MIXED = [("FSK", 0, 8, 3), ("ASK", 70, 100, 1), ("FSK", 5, 10, 2), ("ASK", 0, 8, 3), ("FSK", 70, 100, 1), ("ASK", 5, 100, 7)]


def mixed_params(k):
    return [dp(*[MIXED[i % len(MIXED)][j] for j in (0, 3, 1, 2)]) for i in range(k)]


@pytest.mark.parametrize("policy", [None, "bound", 777])
def test_plan_each_sizes_every_region_from_its_own_parameters(policy):
    from urh_amd import batch
    rng = np.random.default_rng(11)
    for lengths in ([], [12345], [0], [0, 1, 2 ** 31 - 1, 2 ** 31 - 1], list(rng.integers(0, 40000, 200)) + [0, 0, 1, 2, 2 ** 31 - 1]):
        lengths = np.asarray(lengths, dtype=np.int64)
        k = len(lengths)
        params = mixed_params(k)
        table, thr = batch.each_table(params)
        plan, work, blob = batch.batch_plan_each(lengths, table, policy)
        off, rows = plan[:k], plan[k:2 * k]
        tol = np.array([p.tolerance for p in params], dtype=np.int64)
        sps = np.array([p.samples_per_symbol for p in params], dtype=np.int64)
        bound = lengths // (tol + 1) + 2
        want = {None: np.minimum(bound, np.maximum(64, 4 * (lengths // np.maximum(sps, 1)) + 64)), "bound": bound}.get(policy, np.full(k, 777))
        assert np.array_equal(rows, want)
        # ascending, 16-byte aligned, disjoint, each region what THAT capture's (tol, sps, bps) needs
        sizes = np.array([_region_bytes(int(n), int(r), p.samples_per_symbol, p.bits_per_symbol) for n, r, p in zip(lengths, rows, params)], dtype=np.int64)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)[:-1]]) if k else off)
        assert work == int(sizes.sum()) and not (off % 16).any()
        assert blob >= 128 * k and blob % 16 == 0
        assert len(thr) == sum(2 ** p.bits_per_symbol - 1 for p in params)


def test_mixed_sets_side_by_side_have_different_regions():
    from urh_amd import batch
    params = [dp("FSK", 3, 0, 8), dp("FSK", 1, 70, 100)]
    table, _ = batch.each_table(params)
    plan, work, _ = batch.batch_plan_each([20000, 20000], table, "bound")
    a, b = _region_bytes(20000, 20002, 8, 3), _region_bytes(20000, 20000 // 71 + 2, 100, 1)
    assert plan[:2].tolist() == [0, a] and work == a + b and a != b


def test_launch_order_is_partitioned_by_modulation_longest_first():
    from urh_amd import _lib, batch
    rng = np.random.default_rng(3)
    lengths = np.concatenate([rng.integers(0, 5000, 1000), [0, 0, 70001, 70001, 5]]).astype(np.int64)
    params = mixed_params(len(lengths))
    table, _ = batch.each_table(params)
    plan, _, _ = batch.batch_plan_each(lengths, table)
    order = plan[2 * len(lengths):]
    assert sorted(order.tolist()) == list(range(len(lengths)))                  # a permutation
    mods = table["mod"][order]
    n_ask = int((table["mod"] == _lib.MOD_ASK).sum())
    assert (mods[:n_ask] == _lib.MOD_ASK).all() and (mods[n_ask:] == _lib.MOD_FSK).all()
    assert (np.diff(lengths[order[:n_ask]]) <= 0).all() and (np.diff(lengths[order[n_ask:]]) <= 0).all()
    # one modulation: THE longest-first permutation of urhgpu_batch_plan
    table1, _ = batch.each_table([replace(p, modulation_type="FSK") for p in params])
    order1 = batch.batch_plan_each(lengths, table1)[0][2 * len(lengths):]
    assert (np.diff(lengths[order1]) <= 0).all()


@pytest.mark.parametrize("mod,tol,sps,bps", [("FSK", 5, 100, 1), ("ASK", 0, 8, 3), ("FSK", 70, 10, 2)])
def test_a_uniform_table_gives_the_plan_of_one_parameter_set(mod, tol, sps, bps):
    from urh_amd import batch
    rng = np.random.default_rng(tol)
    lengths = np.asarray(list(rng.integers(0, 40000, 300)) + [0, 1, 2, 2 ** 31 - 1], dtype=np.int64)
    p = dp(mod, bps, tol, sps)
    table, _ = batch.each_table([p] * len(lengths))
    for policy in (None, "bound", 31):
        one = batch.batch_plan(lengths, p.to_c(np.dtype(np.float32)), policy)
        each = batch.batch_plan_each(lengths, table, policy)
        assert np.array_equal(one[0], each[0]) and one[1:] == each[1:]


def test_the_table_is_what_a_pass_over_one_capture_derives():
    from urh_amd import _lib, batch
    from urh_amd.signal_functions import get_center_thresholds
    params = [dp("ASK", 2, 3, 10, 0, center=0.37, spacing=0.21), dp("FSK", 1, 65535, 1, 8, center=-0.011), dp("FSK", 7, 0, 8, 2, center=0.1, spacing=0.01)]
    table, thr = batch.each_table(params)
    assert table.dtype.itemsize == 32 and table["mod"].tolist() == [_lib.MOD_ASK, _lib.MOD_FSK, _lib.MOD_FSK]
    assert table["noise_val"].tolist() == [0.0, -4.0, -4.0] and table["thr_first"].tolist() == [0, 3, 4]
    assert table["bits_per_symbol"].tolist() == [2, 1, 7] and table["samples_per_symbol"].tolist() == [10, 1, 8]
    assert table["tolerance"].tolist() == [3, 65535, 0] and table["pause_threshold"].tolist() == [0, 8, 2]
    want = np.concatenate([np.asarray(get_center_thresholds(p.center, p.center_spacing, 2 ** p.bits_per_symbol), dtype=np.float32) for p in params])
    assert np.array_equal(thr.view(np.uint32), want.view(np.uint32))


def test_plan_each_rejects_what_a_batch_does_not_take():
    from urh_amd import _lib, batch
    table, _ = batch.each_table([dp()])
    for bad in ([-1], [2 ** 31]):
        with pytest.raises(_lib.UrhGpuError) as e:
            batch.batch_plan_each(bad, table)
        assert e.value.status == _lib.ERR_ARG
    for field, value, status in (("mod", _lib.MOD_PSK, _lib.ERR_UNSUPPORTED), ("bits_per_symbol", 8, _lib.ERR_UNSUPPORTED), ("bits_per_symbol", 0, _lib.ERR_ARG),
                                 ("samples_per_symbol", 0, _lib.ERR_ARG), ("tolerance", 65536, _lib.ERR_ARG), ("tolerance", -1, _lib.ERR_ARG)):
        t = table.copy()
        t[field] = value
        with pytest.raises(_lib.UrhGpuError) as e:
            batch.batch_plan_each([100], t)
        assert e.value.status == status, field
    with pytest.raises(ValueError, match="one record per capture"):
        batch.batch_plan_each([100, 100], table)


def test_every_refusal_of_the_options():
    from urh_amd.batch import check_batch_each_options
    ps = [dp("ASK"), dp("FSK")]
    assert check_batch_each_options(ps, 2) == ps
    assert check_batch_each_options(ps[0], 3) == [ps[0]] * 3                     # a single DemodParams is broadcast
    assert check_batch_each_options(ps, 2, 8, auto_center=False, dc_correction=False) == ps
    with pytest.raises(ValueError, match=r"not PSK \(params\[1\]\).*iq_to_bits_batch_psk"):
        check_batch_each_options([dp("ASK"), dp("PSK")], 2)
    with pytest.raises(ValueError, match="auto_center is not an option of a batch.*iq_to_bits_batch_center"):
        check_batch_each_options(ps, 2, auto_center=True)
    with pytest.raises(ValueError, match="dc_correction is not an option of a batch.*dc_correct_batch"):
        check_batch_each_options(ps, 2, dc_correction=True)
    with pytest.raises(ValueError, match=r"one DemodParams per capture \(3\).*2 were given"):
        check_batch_each_options(ps, 3)
    for bad in (0, -1, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="message_length_divisor must be at least 1"):
            check_batch_each_options(ps, 2, bad)
    check_batch_each_options(ps, 2, 2 ** 30)
    with pytest.raises(TypeError, match="iq_to_bits_batch_each\\(\\) got an unexpected keyword argument 'msg_records'"):
        check_batch_each_options(ps, 2, msg_records=True)


class _NoDevice:
    """the part of a DevicePipeline the input checks touch before any device work"""
    torch = __import__("torch")          # (pipe.torch: the input forms ask it whether a capture is a tensor)
    _pinned = {}


def test_the_method_refuses_before_a_device_is_touched():
    from urh_amd.batch import iq_to_bits_batch_each
    caps = [np.zeros((10, 2), np.float32), np.zeros((5, 2), np.float32)]
    with pytest.raises(ValueError, match="one DemodParams per capture"):
        iq_to_bits_batch_each(_NoDevice(), caps, [dp()] * 3)
    with pytest.raises(ValueError, match="iq_to_bits_batch_psk"):
        iq_to_bits_batch_each(_NoDevice(), caps, [dp(), dp("PSK")])
    with pytest.raises(ValueError, match="share one sample type"):
        iq_to_bits_batch_each(_NoDevice(), [caps[0], np.zeros((5, 2), np.int8)], [dp()] * 2)


def test_params_from_estimates_on_the_recorded_sessions():
    from urh_amd.batch import params_from_estimates
    sessions = json.load(open(os.path.join(ROOT, "tests", "golden", "batch_estimate", "estimates.json")))
    base = dp("FSK", 1, 5, 100, 8, noise=0.123, center=0.02)
    seen_none = 0
    for name, entries in sessions.items():
        entries = [e for e in entries if not isinstance(e, str)]       # (a string names the exception handing that entry out raises: no entry)
        got = params_from_estimates(entries, base)
        assert len(got) == len(entries)
        for est, p in zip(entries, got):
            if est is None:
                seen_none += 1
                assert p == base
                continue
            assert p.modulation_type == est["modulation_type"] and p.samples_per_symbol == est["bit_length"] and p.tolerance == est["tolerance"]
            assert p.center == est["center"] and p.noise_threshold == est["noise"]
            assert (p.bits_per_symbol, p.pause_threshold, p.center_spacing) == (base.bits_per_symbol, base.pause_threshold, base.center_spacing)
    assert seen_none > 0
    ook = params_from_estimates([{"modulation_type": "OOK", "bit_length": 40, "center": 0.3, "tolerance": 2, "noise": 0.01}], replace(base, bits_per_symbol=2))
    assert (ook[0].modulation_type, ook[0].bits_per_symbol, ook[0].samples_per_symbol) == ("ASK", 1, 40)
    per = params_from_estimates([None, None], [base, replace(base, tolerance=9)])
    assert per[1].tolerance == 9
    with pytest.raises(ValueError, match="one DemodParams per capture"):
        params_from_estimates([None, None], [base])


@pytest.fixture(scope="module")
def each_asm(tmp_path_factory):
    """batch_each.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_host.py does for batch.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch_each") / "batch_each.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_each.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_each_kernels_have_no_spills_and_no_scratch(each_asm):
    kernels = re.findall(r"\.name:\s+(\S*k_batch_\S+)", each_asm)
    assert len(kernels) == 17, kernels           # the walk: five sample types x ASK / FSK; the pack; the records' positions; the RSSI x five sample types
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", each_asm)]
        assert len(values) == 17 and not any(values), (key, values)
    assert "scratch_" not in each_asm


def test_the_walk_holds_no_fp32_fma(each_asm):
    """tests/test_batch_host.py's rule for batch.hip, for the ten per-capture instantiations of the walk (the records' position kernel
    divides integers, which the compiler expands through fp32 -- as in batch_records.hip)"""
    walks = re.findall(r"\n(_ZN3urh12k_batch_bits\w+):[^\n]*\n(.*?)s_endpgm", each_asm, re.S)
    assert len(walks) == 10
    for name, body in walks:
        assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", body), name
        assert not re.search(r"v_div_fixup_f32", body), name
    assert any(re.search(r"v_div_fixup_f64", body) for _, body in walks)
