"""The host side of a batch with an automatic noise threshold per capture (urh_amd/csrc/batch_auto.hip, urh_amd/batch/; include/urhgpu.h
"a batch of captures: automatic noise threshold per capture"): the kernel's summation order against numpy, the model of the whole kernel
against the oracle and the real reference's fixture, the option errors, and the code objects' metadata.  No GPU needed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_auto_cases as bc
import model_batch_noise as mb
import model_noise
import noise_cases as nc


def _full_mantissa(rng, rows, length):
    """the int16 magnitudes: square roots of integers up to 2 * 32767^2 (float32 magnitudes cast to double would sum exactly in ANY order)"""
    return np.sqrt(rng.integers(0, 2 * 32767 ** 2 + 1, (rows, length)).astype(np.float64))


def test_the_kernels_sum_is_numpys_for_every_chunk_length():
    """chunk_sums -- the kernel's additions, one at a time -- equals np.add.reduce bit for bit for every chunk length a default batch can
    meet (1 .. 1966) and longer ones up to a full piece of 8192 terms and beyond it; a plain sequential sum does not"""
    rng = np.random.default_rng(20)
    sequential_differs = 0
    for length in list(range(1, 1967)) + [2047, 2048, 4095, 4096, 4097, 8191, 8192, 8193, 20_000]:
        m = _full_mantissa(rng, 3, length)
        want = np.array([np.add.reduce(np.ascontiguousarray(r)) for r in m])
        got = mb.chunk_sums(m)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), length
        sequential_differs += int((np.cumsum(m, axis=1)[:, -1] != want).sum())      # (np.cumsum adds in order)
    assert sequential_differs > 0              # the inputs can tell the orders apart


def test_the_plan_of_a_piece_stays_inside_the_kernels_arrays():
    """bn_plan's capacities: at most 128 leaves and 256 operations per piece, a value stack and a frame stack of 16 (model_batch_noise.plan
    asserts the frames, chunk_sums the values)"""
    worst = 0
    for length in list(range(1, 1200)) + list(range(8000, 8193)):
        leaves, ops = mb.plan(length)
        assert sum(ln for _, ln in leaves) == length and all(1 <= ln <= mb.PW_LEAF for _, ln in leaves)
        assert [o for o, _ in leaves] == list(np.concatenate([[0], np.cumsum([ln for _, ln in leaves])[:-1]]))
        assert len(ops) == 2 * len(leaves) - 1
        worst = max(worst, len(leaves))
    assert worst <= mb.MAX_LEAVES
    mb.chunk_sums(np.ones((1, 8191)))


def _same(value, want_hex):
    return value.hex() == want_hex


@pytest.mark.parametrize("dtype", nc.DTYPES5, ids=lambda d: np.dtype(d).name)
def test_model_of_the_kernel_against_the_oracle_and_the_reference(oracle, dtype):
    golden = bc.load_golden()
    assert tuple(golden["lengths"]) == bc.SWEEP_LENGTHS
    name = np.dtype(dtype).name
    nonzero = 0
    for i, iq in enumerate(bc.sweep(dtype)):
        mags = mb.magnitudes(iq)
        assert np.array_equal(mags, oracle.get_magnitudes(iq), equal_nan=True)
        noise, flag = mb.detect(iq)
        want, want_flag = nc.oracle_threshold(oracle, iq)
        assert flag == want_flag == 1 and float(noise).hex() == float(want).hex(), (name, len(iq))
        assert _same(float(noise), golden["sweep"][name][i]), (name, len(iq))          # the real reference
        nonzero += noise != 0.0
    assert nonzero == bc.SWEEP_NONZERO[name]


def test_model_of_the_kernel_on_the_flag_captures(oracle):
    golden = bc.load_golden()["flags"]
    seen = {}
    for dtype, caps in ((np.float32, bc.flag_captures_f32()), (np.int8, bc.flag_captures_i8())):
        for name, iq in caps:
            noise, flag = mb.detect(iq)
            want, want_flag = nc.oracle_threshold(oracle, iq)
            assert flag == want_flag, name
            ref = golden[np.dtype(dtype).name][name]
            if flag == 0:
                assert ref == type(want).__name__ == "OverflowError" and math.isinf(noise)
            else:
                assert float(noise).hex() == float(want).hex() == ref, name
            seen[(np.dtype(dtype).name, name)] = (noise, flag)
    assert seen[("float32", "zeros")] == (0.0, 1) and seen[("float32", "constant")] == (0.0, 1) and seen[("float32", "one-nan")] == (0.0, 1)
    assert seen[("float32", "inf")][1] == 0
    assert seen[("float32", "gates-all")] == (4.831, 2) and seen[("int8", "gates-all")] == (181.0194, 2)
    assert 181.0194 > model_noise.max_magnitude(np.int8) > 181.0193
    assert seen[("float32", "clean")] == seen[("float32", "clean-again")] and seen[("float32", "clean")][0] > 0


def test_what_the_automatic_batch_does_not_do_raises_with_a_sentence():
    from urh_amd import batch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)
    batch.check_batch_auto_options(p)
    batch.check_batch_auto_options(p, auto_center=False, msg_records=False, dc_correction=False)
    for name in ("auto_center", "msg_records", "dc_correction"):
        with pytest.raises(ValueError, match="call iq_to_bits"):
            batch.check_batch_auto_options(p, **{name: True})
        with pytest.raises(ValueError, match="call iq_to_bits"):                    # the method checks before it touches a device (None: no pipeline)
            batch.iq_to_bits_batch_auto(None, [], p, **{name: True})
    for mod in ("PSK", "QAM"):
        with pytest.raises(ValueError, match="CaptureStream"):
            batch.iq_to_bits_batch_auto(None, [], DemodParams(mod, 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False))
    with pytest.raises(TypeError):
        batch.check_batch_auto_options(p, no_such_option=1)
    assert callable(DevicePipeline.iq_to_bits_batch_auto) and callable(DevicePipeline.detect_noise_levels)
    # check_batch_options is unchanged: the plain batch still refuses auto_noise, and its sentence now names the new method
    with pytest.raises(ValueError, match="call iq_to_bits") as e:
        batch.check_batch_options(p, auto_noise=True)
    assert "iq_to_bits_batch_auto" in str(e.value)
    with pytest.raises(ValueError, match="call iq_to_bits"):
        batch.iq_to_bits_batch(None, [], p, auto_noise=True)


def test_the_result_sequence_raises_only_where_the_reference_does():
    """BatchBits with noise results: a flag-0 capture raises the reference's exception at [k], at iteration and in check(); the others are
    handed out"""
    from urh_amd.batch import BatchBits

    class Item:
        truncated = False

        def check(self):
            return self
    items = [Item(), Item(), None, Item()]
    res = BatchBits(items, None, [10, 10, 10, 10], noise=[0.5, math.inf, math.nan, 0.0], noise_flags=[1, 0, 0, 1])
    assert res[0] is items[0] and res[3] is items[3] and res[-1] is items[3] and res.noise[0] == 0.5 and res.noise_flags == [1, 0, 0, 1]
    with pytest.raises(OverflowError):
        res[1]
    with pytest.raises(ValueError):
        res[2]
    with pytest.raises(OverflowError):
        res[0:2]
    with pytest.raises(OverflowError):
        res.check()
    it = iter(res)
    assert next(it) is items[0]
    with pytest.raises(OverflowError):
        next(it)
    assert res.truncated == []
    plain = BatchBits(items[:1], None, [10])
    assert plain.noise is None and plain.noise_flags is None and plain.check() is plain and list(plain) == items[:1]


@pytest.fixture(scope="module")
def batch_auto_asm(tmp_path_factory):
    """batch_auto.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_host.py compiles batch.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch_auto") / "batch_auto.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_auto.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_batch_auto_kernels_have_no_spills_and_no_scratch(batch_auto_asm):
    kernels = re.findall(r"\.name:\s+(\S*k_batch_\S+)", batch_auto_asm)
    assert len(kernels) == 25, kernels                      # k_batch_noise per sample type; k_batch_bits with DNOISE: five types x ASK / FSK x order 2 / any
    assert sum("k_batch_noise" in k for k in kernels) == 5
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", batch_auto_asm)]
        assert len(values) == 25 and not any(values), (key, values)
    assert "scratch_" not in batch_auto_asm
    from urh_amd import build
    assert "batch_auto.hip" in build.SOURCES


def test_batch_auto_assembly_holds_no_fp32_fma(batch_auto_asm):
    """the rule of batch.hip, because the same demodulation arithmetic is instantiated here; the float32 magnitudes' square root is taken in
    fp64 and rounded once too (magnitude.hpp takes the translation unit's URH_FSQRT)"""
    assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", batch_auto_asm)
    assert re.search(r"v_div_fixup_f64", batch_auto_asm) and not re.search(r"v_div_fixup_f32", batch_auto_asm)
