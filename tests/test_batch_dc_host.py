"""The host side of the batch's DC correction (urh_amd/batch/ dc_correct_batch, iq_to_bits_batch_dc; include/urhgpu.h "a batch of captures:
DC correction per capture"): the option errors, raised before a device is touched; the older entry points' refusals, which now name the new
method; the C ABI's refusals; the conditions on the inputs of tests/test_batch_dc_gpu.py, checked with the oracle; and the code objects'
metadata of batch_dc.hip.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import batch_dc_cases as cases


def _p(mod="FSK", bps=1):
    from urh_amd.pipeline import DemodParams
    return DemodParams(mod, bps, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)


def test_the_new_methods_check_before_they_touch_a_device():
    from urh_amd import batch, protocol
    from urh_amd.pipeline import DevicePipeline
    assert callable(DevicePipeline.iq_to_bits_batch_dc) and callable(DevicePipeline.dc_correct_batch)
    for mod in ("FSK", "ASK", "PSK"):
        batch.check_batch_dc_options(_p(mod))
        batch.check_batch_dc_options(_p(mod), 8)
    for name in ("no_such_option", "msg_records", "dc_correction", "auto_noises"):
        with pytest.raises(TypeError, match=name):
            batch.check_batch_dc_options(_p(), **{name: True})
        with pytest.raises(TypeError, match=name):
            batch.iq_to_bits_batch_dc(None, [], _p(), **{name: True})          # (None: no pipeline)
    for divisor in (0, -1, (1 << 30) + 1):
        with pytest.raises(ValueError, match="message_length_divisor"):
            batch.check_batch_dc_options(_p(), divisor)
        with pytest.raises(ValueError, match="message_length_divisor"):
            batch.iq_to_bits_batch_dc(None, [], _p("ASK"), message_length_divisor=divisor)
    with pytest.raises(ValueError):
        batch.iq_to_bits_batch_dc(None, [], _p("QAM"))
    import inspect
    assert inspect.signature(protocol.get_protocols_from_signals_dev).parameters["dc_correction"].default is False


def test_the_five_older_entry_points_still_refuse_and_name_the_new_method():
    from urh_amd import batch
    calls = (lambda: batch.iq_to_bits_batch(None, [], _p(), dc_correction=True), lambda: batch.iq_to_bits_batch_auto(None, [], _p(), dc_correction=True),
             lambda: batch.iq_to_bits_batch_center(None, [], _p(), dc_correction=True), lambda: batch.iq_to_bits_batch_records(None, [], _p(), dc_correction=True),
             lambda: batch.iq_to_bits_batch_psk(None, [], _p("PSK"), dc_correction=True))
    for call in calls:
        with pytest.raises(ValueError, match="a batch does not remove the captures' means: call iq_to_bits\\(") as e:
            call()
        s = str(e.value)
        assert "dc_correction is not an option of a batch" in s and "CaptureStream" in s
        assert "iq_to_bits_batch_dc" in s and s.index("iq_to_bits_batch_dc") < s.index("a batch does not remove")


def test_c_abi_refusals_without_a_gpu():
    """the prototype exists; what is rejected before any device work"""
    from urh_amd import _lib
    lib = _lib.load()
    assert "urhgpu_batch_dc_correct_dev" in _lib.PROTOTYPES and hasattr(lib, "urhgpu_batch_dc_correct_dev")
    null, ctx = C.c_void_p(None), C.c_void_p(0x1000)         # (never followed: every call below is refused before the context is used)
    a, b, s, pl = (C.c_void_p(v) for v in (0x10000, 0x20000, 0x30000, 0x40000))

    def call(d_iq=a, total=64, dtype=_lib.DT_F32, d_start=s, d_plan=pl, k=1, d_out=b, d_mean=null, c=ctx):
        return lib.urhgpu_batch_dc_correct_dev(c, d_iq, total, dtype, d_start, d_plan, k, d_out, d_mean)
    assert call(c=null) == _lib.ERR_ARG
    assert call(k=-1) == _lib.ERR_ARG and call(total=-1) == _lib.ERR_ARG
    for dtype in (-1, 5, 7):
        assert call(dtype=dtype) == _lib.ERR_DTYPE
    assert call(d_start=null) == _lib.ERR_ARG and call(d_plan=null) == _lib.ERR_ARG
    assert call(d_iq=null) == _lib.ERR_ARG and call(d_out=null) == _lib.ERR_ARG
    assert call(d_iq=C.c_void_p(0x10004)) == _lib.ERR_ARG                          # half a sample
    assert call(d_out=C.c_void_p(0x20008)) == _lib.ERR_ARG                         # a sample, but not 16 bytes
    assert call(d_mean=C.c_void_p(0x50004)) == _lib.ERR_ARG
    assert call(d_out=C.c_void_p(0x10000 + 64 * 8 - 16)) == _lib.ERR_ARG           # overlaps the input's last two samples
    assert call(d_out=C.c_void_p(0x10000 + 64 * 2 - 16), dtype=_lib.DT_I8) == _lib.ERR_ARG
    assert call(k=0) == _lib.OK and call(k=0, d_out=a) == _lib.OK                  # nothing to launch: nothing is touched


def test_the_inputs_meet_their_conditions(oracle):
    """every numpy-corrected capture of the demodulation sets gives a pulse table of more than 10 rows; at least four of the six captures of
    each ASK set give other bits without the correction -- by the oracle alone"""
    for kind in cases.SETS:
        caps, p, dtype, options, corrected = cases.demod_set(kind)
        assert len(caps) == 6 and all(8_193 <= len(c) <= 40_000 and c.dtype == dtype for c in caps)
        differ = 0
        for c, x in zip(caps, corrected):
            pp, bits = cases.oracle_bits(oracle, x, p, options)
            assert len(pp) > 10, (kind, len(c), len(pp))
            if kind in cases.ASK_SETS:
                raw = cases.oracle_bits(oracle, c, p, options)[1]
                differ += not np.array_equal(raw, bits)
        if kind in cases.ASK_SETS:
            assert differ >= 4, (kind, differ)
    for dtype in cases.DTYPES:
        caps, cat, starts, want = cases.sweep(dtype)
        lengths = [len(c) for c in caps]
        assert len(caps) == cases.SWEEP_K > 64 and set(cases.SWEEP_FIXED) <= set(lengths) and lengths != sorted(lengths, reverse=True)
        assert starts[0] == 3 and len(cat) == starts[-1] + 5
        assert np.isnan(want[lengths.index(0)][1]).all()
    caps, want = cases.int_values("uint16_wrap")
    below = caps[0][:, 0] < want[0][1][0]
    assert below.any() and (want[0][0][below, 0] > 32768).all()                    # the case does wrap


@pytest.fixture(scope="module")
def batch_dc_asm(tmp_path_factory):
    """batch_dc.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_host.py does for batch.hip"""
    from urh_amd import build
    assert "batch_dc.hip" in build.SOURCES
    out = str(tmp_path_factory.mktemp("batch_dc") / "batch_dc.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_dc.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_batch_dc_kernels_have_no_spills_no_scratch_and_fit_the_lds(batch_dc_asm):
    """the code object's metadata of every kernel of batch_dc.hip -- the mean and the subtraction for the five sample types --: no spilled
    vector or scalar registers, no private segment, less than 64 KiB of LDS"""
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", batch_dc_asm.split("amdhsa.kernels:")[1]) if "k_batch_dc_" in b]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    assert len(blocks) == 10 and sum("k_batch_dc_mean" in n for n in names) == 5 and sum("k_batch_dc_sub" in n for n in names) == 5, names
    for name, b in zip(names, blocks):
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert int(re.search(r"\." + key + r":\s+(\d+)", b).group(1)) == 0, (name, key)
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1)) < 65536, name
