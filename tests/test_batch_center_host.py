"""The host side of a batch with an automatic center per capture (urh_amd/csrc/batch_center.hip, urh_amd/batch/; include/urhgpu.h "a
batch of captures: automatic center per capture"): the option errors, the size / plan call against a restatement, the numpy model of the
pass against the oracle and the real reference's fixture, the slicing thresholds against the library's host arithmetic, and the code
objects' metadata.  No GPU needed."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_center_cases as B
import center_cases as cc
import model_batch_center as mc
import noise_cases as nc


def test_option_sentences_and_type_errors():
    from urh_amd import batch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
    batch.check_batch_center_options(p)
    batch.check_batch_center_options(p, msg_records=False, dc_correction=False)
    for name in ("msg_records", "dc_correction"):
        with pytest.raises(ValueError, match="call iq_to_bits"):
            batch.check_batch_center_options(p, **{name: True})
        with pytest.raises(ValueError, match="call iq_to_bits"):                    # checked before a device is touched (None: no pipeline)
            batch.iq_to_bits_batch_center(None, [], p, **{name: True})
    for mod in ("PSK", "QAM"):
        with pytest.raises(ValueError, match="CaptureStream"):
            batch.iq_to_bits_batch_center(None, [], DemodParams(mod, 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False))
    with pytest.raises(TypeError):
        batch.check_batch_center_options(p, auto_center=True)                       # (not an option here: it is what the method does)
    with pytest.raises(TypeError):
        batch.iq_to_bits_batch_center(None, [], p, no_such_option=1)
    for name in ("iq_to_bits_batch_center", "detect_centers", "qad_to_bits_batch"):
        assert callable(getattr(DevicePipeline, name))
    # the old methods still raise for auto_center=True, and their sentences name the new method
    for check, call in ((batch.check_batch_options, batch.iq_to_bits_batch), (batch.check_batch_auto_options, batch.iq_to_bits_batch_auto)):
        with pytest.raises(ValueError, match="call iq_to_bits") as e:
            check(p, auto_center=True)
        assert "iq_to_bits_batch_center" in str(e.value)
        with pytest.raises(ValueError, match="call iq_to_bits"):
            call(None, [], p, auto_center=True)


def test_the_result_sequence_carries_centers_and_flags():
    from urh_amd.batch import BatchBits
    res = BatchBits([object(), object()], None, [10, 10], centers=[0.25, None], center_flags=[3, 0])
    assert res.centers == [0.25, None] and res.center_flags == [3, 0] and res.noise is None
    assert BatchBits([], None, []).centers is None


def test_plan_against_a_restatement():
    from urh_amd import _lib, batch
    rng = np.random.default_rng(3)
    for k, bins in ((0, 4096), (1, 4096), (3, 4096), (4095, 4096), (4096, 4096), (4097, 4096), (8193, 4096), (5000, 64), (7, 1), (2, 1 << 20), (17, 1 << 20),
                    (262144, 64), (262145, 64)):
        lengths = rng.integers(0, 300, k)
        total = int(lengths.sum())
        assert batch.batch_center_plan(lengths, None, bins) == mc.plan(k, total, bins), (k, bins)
        assert batch.batch_center_plan(lengths, total + 1000, bins) == mc.plan(k, total + 1000, bins)
    # the group count either side of the pool limit: K x bins x 4 bytes against 64 MiB
    assert batch.batch_center_plan(np.zeros(4096, np.int64), None, 4096)[1:] == (1, 4096)
    assert batch.batch_center_plan(np.zeros(4097, np.int64), None, 4096)[1:] == (2, 4096)
    assert batch.batch_center_plan(np.zeros(16, np.int64), None, 1 << 20)[1:] == (1, 16)
    assert batch.batch_center_plan(np.zeros(17, np.int64), None, 1 << 20)[1:] == (2, 16)
    lib = _lib.load()
    out = C.c_int64(0)
    bad = np.array([5, -1], np.int64)
    assert lib.urhgpu_batch_center_plan(bad.ctypes.data_as(C.c_void_p), 2, -1, 4096, C.byref(out), None, None) == _lib.ERR_ARG
    assert lib.urhgpu_batch_center_plan(None, 2, -1, 4096, C.byref(out), None, None) == _lib.ERR_ARG
    assert lib.urhgpu_batch_center_plan(None, 2, 100, 0, C.byref(out), None, None) == _lib.ERR_ARG
    assert lib.urhgpu_batch_center_plan(None, 2, 100, 4096, C.byref(out), None, None) == 0 and out.value == mc.plan(2, 100, 4096)[0]


def test_thresholds_are_the_librarys_host_arithmetic():
    from urh_amd import _lib, batch
    from urh_amd.pipeline import DemodParams
    lib = _lib.load()
    rng = np.random.default_rng(4)
    for bps in (1, 2, 3, 7):
        order = 1 << bps
        p = DemodParams("FSK", bps, 0.0, 0.123456789, 0.0371, 5, 100, 0.1, 8, False)
        centers = [None] + [float(x) for x in rng.normal(0, 0.3, 20)] + [1e-30, -3.0000001]
        got = batch.center_thresholds(p, centers)
        assert got.shape == (len(centers), order - 1) and got.dtype == np.float32
        for c, row in zip(centers, got):
            want = np.zeros(order - 1, np.float32)
            lib.urhgpu_get_center_thresholds(p.center if c is None else c, p.center_spacing, order, want.ctypes.data_as(C.c_void_p))
            assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), (bps, c)


@pytest.mark.parametrize("dtype", B.GAIN_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("mod", B.GAIN_MODS)
def test_model_on_the_gain_sweep_against_the_oracle_and_the_reference(oracle, mod, dtype):
    name = np.dtype(dtype).name
    golden = B.load_golden()
    p = B.gain_params(mod)
    seen = collections.Counter()
    for max_size in B.GAIN_MAX_SIZES:
        g = golden["%s/%s/%s" % (mod, name, max_size)]
        per = collections.Counter()
        for i, iq in enumerate(B.gain_sweep(mod, dtype)):
            m = mc.capture(oracle, iq, p, max_size)
            r = B.reference(oracle, iq, p, max_size, True, key=("gain-host", mod, name, i))
            assert m["noise_flag"] == r[1] == 1 and m["noise"] == r[0]                # every capture of the sweep has noise flag 1
            c = oracle.detect_center(m["qad"], max_size)
            assert (c is None and m["center"] is None) or float(c) == m["center"] == r[2][0], (i, c, m["center"])
            cls = B.expected_class(r, max_size)
            assert m["flag"] == cc.FLAG[cls]
            assert np.array_equal(m["pp"], r[2][2]) and np.array_equal(m["flat"][0], r[2][3]) and np.array_equal(m["flat"][2], r[2][5])
            # the real reference's record
            assert g["class"][i] == cls and g["center"][i] == (None if m["center"] is None else m["center"].hex()), (i, g["center"][i], m["center"])
            assert g["hash"][i] == B.ref_hash(r), i
            per[cls] += 1
        seen.update(per)
    assert dict(seen) == B.GAIN_CLASSES[(mod, name)]
    # conditions, not tolerances: the sweep exercises every class it is meant to.  They hold per (modulation, sample type) over the 256
    # outcomes of BOTH max_size values together -- at max_size None alone an ASK float32 batch is 128 decided captures and has neither a
    # `none` nor a `tie`; those come from the cut to 1000 samples
    if mod == "ASK":
        assert seen["ok"] >= 128 and seen["none"] >= 1 and seen["tie"] >= 1
    else:
        assert seen["ok"] >= 10 and seen["tie"] >= 10


def test_model_on_the_flag_captures_against_the_reference(oracle):
    """batch_auto_cases.flag_captures_f32 against the real reference's record; the constant envelope's record is only read here (166
    million bins: numpy takes a minute over its histogram) -- the GPU test holds the batch against it"""
    import batch_auto_cases as bac
    golden = B.load_golden()["flags"]
    p = nc.params("FSK", 1, write_pos=False)
    for name, iq in bac.flag_captures_f32():
        g = golden[name]
        if name == "constant":
            assert g["class"] == "wide" and float.fromhex(g["noise"]) == 0.0 and abs(float.fromhex(g["center"]) - 2 * np.pi / 100) < 1e-6
            continue
        m = mc.capture(oracle, iq, p, None)
        if m["noise_flag"] == 0:
            assert g["noise"] == type(m["noise"]).__name__ == "OverflowError"
            continue
        assert float(m["noise"]).hex() == float.fromhex(g["noise"]).hex(), name
        assert (m["center"] is None and g["center"] is None) or m["center"].hex() == float.fromhex(g["center"]).hex(), name
        assert m["flag"] == cc.FLAG[g["class"]] and B.bits_hash(*nc.messages_of(m["flat"])) == g["hash"], name
        assert (m["noise_flag"] == 2) == (name == "gates-all")


def test_the_center_moves_the_slicing_on_the_gain_sweep(oracle):
    """the reason for the method: sliced with the capture's own center, the pulse table differs from the one sliced with the shared center"""
    for mod, least in (("ASK", 120), ("FSK", 50)):
        p = B.gain_params(mod)
        differ, centers = 0, []
        for i, iq in enumerate(B.gain_sweep(mod, np.float32)):
            r = B.reference(oracle, iq, p, None, True, key=("gain-host", mod, "float32", i))
            if r[2][0] is None:
                continue
            centers.append(r[2][0])
            pp, _ = nc.slice_qad(oracle, r[2][1], p)
            differ += not np.array_equal(pp, r[2][2])
        assert differ >= least, (mod, differ)
        if mod == "ASK":
            assert min(centers) < 0.002 and max(centers) > 0.17


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_model_on_the_geometry_sweep_against_the_oracle(oracle, dtype):
    for mod in cc.MODS:
        p = B.geometry_params(mod, dtype)
        for auto_noise in (True, False):
            for iq in B.geometry_sweep(dtype)[1:-1]:
                for max_size in cc.MAX_SIZES:
                    m = mc.capture(oracle, iq, p, max_size, auto_noise)
                    assert m["noise_flag"] in (1, 2)
                    c = oracle.detect_center(m["qad"], max_size)
                    assert (c is None and m["center"] is None) or float(c) == m["center"], (mod, len(iq), max_size, c, m["center"])
                    assert m["flag"] == cc.FLAG[cc.expected(m["qad"], max_size)]
                    if len(iq) <= 2:
                        assert m["center"] is None and not m["qad"].any()


@pytest.fixture(scope="module")
def batch_center_asm(tmp_path_factory):
    """batch_center.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_auto_host.py compiles batch_auto.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch_center") / "batch_center.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_center.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_batch_center_kernels_have_no_spills_and_no_scratch(batch_center_asm):
    kernels = re.findall(r"\.name:\s+(\S*k_batch_\S+)", batch_center_asm)
    # k_batch_demod: five types x ASK / FSK x DNOISE; k_batch_bits with a qad input: ASK / FSK x order 2 / any; k_batch_center_publish
    assert len(kernels) == 25, kernels
    assert sum("k_batch_demod" in k for k in kernels) == 20 and sum("k_batch_bits" in k for k in kernels) == 4
    assert sum("k_batch_center_publish" in k for k in kernels) == 1
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", batch_center_asm)]
        assert len(values) == 25 and not any(values), (key, values)
    from urh_amd import build
    assert "batch_center.hip" in build.SOURCES


def test_batch_center_assembly_holds_no_fp32_fma(batch_center_asm):
    """the rule of batch.hip, because the same demodulation arithmetic is instantiated here"""
    assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", batch_center_asm)
    assert re.search(r"v_div_fixup_f64", batch_center_asm) and not re.search(r"v_div_fixup_f32", batch_center_asm)
