"""The device-driven re-speculation of the Costas loop (urh_amd/csrc/costas.hip), checked without a GPU: the round kernels that read their
round from the control block cost no more registers than the ones that take it as arguments, and the scratch a pass reserves covers the
control block."""
import ctypes as C
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel symbol: {metadata key: value}} of costas.hip compiled device-only for gfx950"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("costas") / "costas.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "costas.hip"), "-o", out], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    found = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        named = re.search(r"\n    \.name:\s+(\S+)", block)
        if not named:                                        # (the version numbers behind the kernels)
            continue
        name = named.group(1)
        found[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))
                       for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "vgpr_count", "sgpr_count")}
    return found


def test_device_driven_round_kernels_cost_no_more_than_their_twins(kernels):
    # the DEV flag is the last template argument of k_costas_spec / k_costas_stitch (after SH = false) and the only one of k_costas_map
    pairs = []
    for name in kernels:
        if re.search(r"k_costas_(spec|stitch)ILi\d+ELi\dELb0ELb1EE", name):
            pairs.append((name, name.replace("ELb0ELb1EE", "ELb0ELb0EE")))
        elif "k_costas_mapILb1EE" in name:
            pairs.append((name, name.replace("k_costas_mapILb1EE", "k_costas_mapILb0EE")))
    assert len(pairs) == 2 * 5 * 2 + 1, sorted(kernels)      # spec and stitch: five sample types x two loop orders; one map
    for dev, twin in pairs:
        assert twin in kernels, twin
        for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert kernels[dev][key] <= kernels[twin][key], (dev, key, kernels[dev], kernels[twin])


def test_scratch_covers_the_control_block():
    from urh_amd import _lib
    lib = _lib.load()
    out = (C.c_int64 * 3)()
    for n in (8193, 8200, 3 * 4096, 3 * 4096 + 1, 3 * 4096 + 2, 70_001, 300_000, (1 << 20) + 4096, 1 << 27, (1 << 31) - 1):
        for order in (2, 4):
            assert lib.urhgpu_test_costas_scratch(n, order, out) == 0
            scratch, ctl_end, ctl_bytes = (int(v) for v in out)
            assert ctl_bytes >= 8 + 4 + 4 + 4 + 4 and ctl_end <= scratch, (n, order, scratch, ctl_end)
    assert lib.urhgpu_test_costas_scratch(100, 3, out) == _lib.ERR_ARG
