"""The host side of the PSK batch (urh_amd/batch/ iq_to_bits_batch_psk, costas_demod_batch; include/urhgpu.h "a batch of captures: PSK"):
the option errors, raised before a device is touched; the older entry points' refusals, which now name the new method; the C ABI's
refusals; and the code objects' metadata of k_batch_costas.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest


def _p(mod="PSK", bps=2):
    from urh_amd.pipeline import DemodParams
    return DemodParams(mod, bps, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)


def test_the_new_method_checks_before_it_touches_a_device():
    from urh_amd import batch
    from urh_amd.pipeline import DevicePipeline
    assert callable(DevicePipeline.iq_to_bits_batch_psk) and callable(DevicePipeline.costas_demod_batch)
    batch.check_batch_psk_options(_p(), dc_correction=False)
    batch.check_batch_psk_options(_p(), 8)
    for mod in ("FSK", "ASK", "QAM"):
        for call in (lambda p: batch.iq_to_bits_batch_psk(None, [], p), lambda p: batch.costas_demod_batch(None, [], p)):
            with pytest.raises(ValueError, match="iq_to_bits_batch") as e:
                call(_p(mod))
            for sibling in ("iq_to_bits_batch_auto", "iq_to_bits_batch_center", "iq_to_bits_batch_records"):
                assert sibling in str(e.value)
    with pytest.raises(ValueError, match="does not remove the captures' means") as e:
        batch.iq_to_bits_batch_psk(None, [], _p(), dc_correction=True)
    assert "call iq_to_bits(" in str(e.value) and "CaptureStream" in str(e.value)
    for name in ("no_such_option", "msg_records", "auto_noises"):
        with pytest.raises(TypeError, match=name):
            batch.iq_to_bits_batch_psk(None, [], _p(), **{name: True})
    for divisor in (0, -1, (1 << 30) + 1):
        with pytest.raises(ValueError, match="message_length_divisor"):
            batch.iq_to_bits_batch_psk(None, [], _p(), message_length_divisor=divisor)


def test_the_older_entry_points_still_refuse_psk_and_name_the_new_method():
    from urh_amd import _lib, batch
    calls = (lambda p: batch.check_batch_options(p), lambda p: batch.iq_to_bits_batch(None, [], p), lambda p: batch.iq_to_bits_batch_auto(None, [], p),
             lambda p: batch.iq_to_bits_batch_center(None, [], p), lambda p: batch.iq_to_bits_batch_records(None, [], p),
             lambda p: batch.qad_to_bits_batch(None, (np.zeros(4, np.float32), [0, 4]), p))
    for call in calls:
        with pytest.raises(ValueError, match="CaptureStream") as e:
            call(_p())
        assert "iq_to_bits_batch_psk" in str(e.value)
    with pytest.raises(_lib.UrhGpuError) as e:
        batch.batch_plan([100], _p().to_c(np.float32))
    assert e.value.status == _lib.ERR_UNSUPPORTED
    # ... and a PSK batch is planned with the parameters recoded as FSK: the plan reads lengths, tolerance, samples and bits per symbol alone
    a = batch.batch_plan([100, 7, 4000], batch.as_fsk(_p()).to_c(np.float32))
    b = batch.batch_plan([100, 7, 4000], _p("FSK").to_c(np.float32))
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and batch.as_fsk(_p("ASK")).modulation_type == "ASK"


def test_c_abi_refusals_without_a_gpu():
    """the prototypes exist; what is rejected before any device work"""
    from urh_amd import _lib
    lib = _lib.load()
    for name in ("urhgpu_batch_costas_dev", "urhgpu_iq_to_bits_batch_psk_dev"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    null = C.c_void_p(None)
    ctx = C.c_void_p(0x1000)                   # (never followed: every call below is refused before the context is used)

    def costas(p, dtype=np.float32, k=0, d_qad=null):
        return lib.urhgpu_batch_costas_dev(ctx, null, 0, null, null, k, C.byref(p.to_c(dtype)), null, d_qad)
    assert lib.urhgpu_batch_costas_dev(null, null, 0, null, null, 0, C.byref(_p().to_c(np.float32)), null, null) == _lib.ERR_ARG
    assert lib.urhgpu_batch_costas_dev(ctx, null, 0, null, null, 0, None, null, null) == _lib.ERR_ARG
    for mod in ("FSK", "ASK", "QAM"):
        assert costas(_p(mod)) == _lib.ERR_UNSUPPORTED
    assert costas(_p(bps=8)) == _lib.ERR_UNSUPPORTED
    cp = _p().to_c(np.float32)
    cp.mod_order = 3                            # a loop order the reference writes no output for
    assert lib.urhgpu_batch_costas_dev(ctx, null, 0, null, null, 0, C.byref(cp), null, null) == _lib.ERR_UNSUPPORTED
    assert costas(_p(), k=-1) == _lib.ERR_ARG
    assert costas(_p(), k=1) == _lib.ERR_ARG                                        # starts and plan are missing
    assert costas(_p(), d_qad=C.c_void_p(0x1002)) == _lib.ERR_ARG                   # misaligned output

    def whole(p, d_qad=C.c_void_p(0x2000)):
        return lib.urhgpu_iq_to_bits_batch_psk_dev(null, null, 0, null, null, 0, C.byref(p.to_c(np.float32)), 0, 0, -1, d_qad, null, 0, null, null, null, 0, null,
                                                   null, 0, null, 0, null, 0, null, 0)
    assert whole(_p(), d_qad=null) == _lib.ERR_ARG                                  # the demodulated buffer is required
    for mod in ("FSK", "ASK", "QAM"):
        assert whole(_p(mod)) == _lib.ERR_UNSUPPORTED
    assert whole(_p()) == _lib.ERR_ARG                                              # everything in order but the context


@pytest.fixture(scope="module")
def batch_psk_asm(tmp_path_factory):
    """batch_psk.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_host.py does for batch.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch_psk") / "batch_psk.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_psk.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_batch_costas_kernels_have_no_spills_no_scratch_and_fit_the_lds(batch_psk_asm):
    """the code object's metadata of every k_batch_costas instantiation -- five sample types x loop order 2 / 4 x with / without per-capture
    noise blocks --: no spilled vector or scalar registers, no private segment, the two tiles within 64 KiB of LDS"""
    blocks = [b for b in re.split(r"\n  - \.agpr_count:", batch_psk_asm.split("amdhsa.kernels:")[1]) if "k_batch_costas" in b]
    assert len(blocks) == 20, len(blocks)
    for b in blocks:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert int(re.search(r"\." + key + r":\s+(\d+)", b).group(1)) == 0, (name, key)
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", b).group(1))
        assert 64 * 65 * 12 <= lds <= 65536, (name, lds)
