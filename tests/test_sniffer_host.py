"""urh_amd.sniffer.LiveSniffer's state machine against the reference's recorded live runs (tests/golden/sniffer/, made by
tests/golden/make_sniffer_golden.py from ProtocolSniffer.__demodulate_data), with the numpy engine of tests/model_sniffer.py:
no GPU needed.  Every per-chunk record (above-noise flag, noise threshold as value AND scalar type, pause_length, buffer index)
and every message (bits, pause, first bit position, timestamp at the fixed clock) must be equal."""
import numpy as np
import pytest

import model_sniffer as ms

EXPECTED_CASES = ["ask_f32_autocenter", "fsk4_f32", "fsk_f32_adaptive_autocenter", "fsk_f32_small_buffer", "fsk_f32_tiny_chunks",
                  "fsk_i16_adaptive", "fsk_i8_adaptive", "fsk_u16", "fsk_u8", "psk_f32"]


def test_every_fixture_is_there():
    assert ms.SNIFFER_CASES == EXPECTED_CASES


@pytest.mark.parametrize("name", EXPECTED_CASES)
def test_fixture_is_not_hollow(name):
    g = ms.load_case(name)
    unsigned = g["iq"].dtype.kind == "u"
    assert len(g["pauses"]) >= (1 if unsigned else 3) and len(g["centers"]) >= 1
    assert int(g["chunk_lens"].sum()) == len(g["iq"])
    if g["adaptive_noise"]:
        assert len(set(g["rec_noise"].tolist())) > 1
        assert str(g["rec_noise_type"][-1]) == ("float32" if g["iq"].dtype == np.float32 else "float64")
    else:
        assert set(g["rec_noise_type"].tolist()) == {"float"}
    if name == "fsk_f32_small_buffer":
        assert g["n_trims"] >= 1
    if name == "fsk_f32_tiny_chunks":
        assert (g["chunk_lens"] == 0).sum() >= 2 and ((g["chunk_lens"] > 0) & (g["chunk_lens"] < 8)).sum() >= 100


@pytest.mark.parametrize("name", EXPECTED_CASES)
def test_sniffer_equals_reference(name, oracle):
    g = ms.load_case(name)
    sniffer = ms.make_sniffer(g, ms.NumpySniffEngine(g["iq"].dtype, g["buffer_samples"]))
    ms.check_against_fixture(g, sniffer, ms.chunks_of(g))


def test_noise_threshold_keeps_the_reference_scalar_types():
    """NEP 50: the Python constants are weak, so the first adaptive update turns the threshold into the chunk's numpy float type; an update
    that does not change the value is dropped by Signal.noise_threshold's setter and the type stays"""
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import LiveSniffer
    for dtype, name in ((np.float32, "float32"), (np.int8, "float64")):
        sn = LiveSniffer(None, DemodParams("FSK", 1, 0.0, 0.0), dtype=dtype, adaptive_noise=True, buffer_samples=1000,
                         engine=ms.NumpySniffEngine(dtype, 1000), trace=True)
        sn.feed(np.zeros((10, 2), dtype))
        assert type(sn.noise_threshold) is float and sn.noise_threshold == 0.0          # 0.9 * 0 + 0.1 * 0 == 0: not assigned
        sn.noise_threshold = 5.0
        sn.feed(np.ones((10, 2), dtype))
        assert type(sn.noise_threshold).__name__ == name and float(sn.noise_threshold) == float(0.9 * 5.0 + 0.1 * np.sqrt(np.asarray(1, dtype) ** 2.0))


def test_clear_and_empty_chunk():
    from urh_amd.pipeline import DemodParams
    from urh_amd.sniffer import LiveSniffer
    sn = LiveSniffer(None, DemodParams("FSK", 1, 0.1, 0.0), buffer_samples=1000, engine=ms.NumpySniffEngine(np.float32, 1000), trace=True)
    assert sn.feed(np.zeros((0, 2), np.float32)) == [] and sn.index == 0 and sn.trace[-1]["above"] is None
    sn.feed(np.ones((10, 2), np.float32))
    assert sn.index == 10 and sn.pause_length == 0
    sn.clear()
    assert sn.index == 0 and sn.messages == []


def test_chunk_kernels_have_no_spills_and_no_scratch(tmp_path):
    """the code object's metadata of every kernel in chunk_stats.hip, compiled for gfx950 (no GPU needed): no spilled registers, no private
    segment"""
    import os
    import re
    import subprocess
    from conftest import ROOT
    from urh_amd import build
    out = str(tmp_path / "chunk_stats.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "chunk_stats.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    txt = open(out).read()
    kernels = re.findall(r"\.name:\s+(\S*k_chunk_\S+)", txt)
    assert len(kernels) == 7, kernels                        # f32 + four integer types, two finish kernels
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", txt)]
        assert len(values) == 7 and not any(values), (key, values)
    assert "scratch_" not in txt
    assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", txt)       # the squares do not fuse into the adds
