"""Automatic center inside a pass (include/urhgpu.h: urhgpu_detect_center_dev, urhgpu_iq_to_bits_auto_center_dev, urhgpu_stream_set_auto_center /
urhgpu_stream_center), the parts that need no GPU: the ABI, its argument errors, and what the GPU tests' sweep (center_cases.py)
rests on -- most cases are decided on the device, and the hand-out path for the others (numpy on the shipped histogram) gives the
reference's center."""
import ctypes as C
import os
import re

import numpy as np

import center_cases as cc
from conftest import ROOT

NEW = ("urhgpu_detect_center_dev", "urhgpu_iq_to_bits_auto_center_dev", "urhgpu_center_hist_cap", "urhgpu_stream_set_auto_center", "urhgpu_stream_center",
       "urhgpu_test_center_host_syncs")


def test_new_symbols_are_declared_exported_and_prototyped():
    from urh_amd import _lib, build
    build.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "urhgpu.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert "typedef struct urhgpu_center_result" in header and C.sizeof(_lib.CenterResult) == 64
    assert '"auto_center_max_bins"' in open(os.path.join(ROOT, "include", "urhgpu.h")).read()
    assert _lib.load().urhgpu_version() == 100


def test_abi_layout_of_the_old_structs_is_unchanged():
    from urh_amd import _lib
    assert (C.sizeof(_lib.Params), C.sizeof(_lib.Outputs), C.sizeof(_lib.HostResult)) == (64, 120, 176)


def test_argument_errors():
    from urh_amd import _lib
    lib = _lib.load()
    null = C.c_void_p(None)
    buf = (C.c_char * 4096)()                                 # host memory standing in for device pointers: the calls are rejected before any device work
    fake = C.cast(buf, C.c_void_p)
    p = cc.params("FSK", np.float32).to_c(np.float32)
    o = _lib.Outputs()
    assert lib.urhgpu_detect_center_dev(null, fake, 100, -1, fake, 0) == _lib.ERR_ARG
    # a null context, with complete outputs and with out->qad == NULL (a real context with out->qad == NULL: test_auto_center_gpu.py)
    o.rows, o.counts, o.cap_rows, o.qad = fake.value, fake.value, 16, fake.value
    assert lib.urhgpu_iq_to_bits_auto_center_dev(null, fake, 100, C.byref(p), -1, C.byref(o), fake, null, 0) == _lib.ERR_ARG
    o.qad = None
    assert lib.urhgpu_iq_to_bits_auto_center_dev(null, fake, 100, C.byref(p), -1, C.byref(o), fake, null, 0) == _lib.ERR_ARG
    assert lib.urhgpu_stream_set_auto_center(null, 1, 7500) == _lib.ERR_ARG
    assert lib.urhgpu_stream_center(null, 0, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.urhgpu_center_hist_cap(null) == 0
    assert lib.urhgpu_ctx_set_tuning(null, b"auto_center_max_bins", 8) == _lib.ERR_ARG
    assert lib.urhgpu_test_center_host_syncs() >= 0
    assert not hasattr(lib, "urhgpu_center_note_host_syncs")      # the counter has no writer outside the library


def test_most_of_the_sweep_is_decided_on_the_device(oracle):
    """the condition the GPU tests rest on: at least 80 % of the sweep's cases are 'ok' (decided on the device, flag 1)"""
    kinds = [cc.expected(cc.sweep_qad(oracle, n, dt, mod), ms) for mod, dt, n, ms in cc.sweep()]
    count = {k: kinds.count(k) for k in ("ok", "tie", "none", "wide")}
    print("sweep:", count)
    assert len(kinds) == 400
    assert count["ok"] >= 0.8 * len(kinds), count
    assert count["tie"] >= 1, count                          # the hand-out path is exercised too


def test_expected_agrees_with_the_oracle_on_none(oracle):
    """'none' <=> oracle.detect_center returns None (wide aside), on the sweep and on the degenerate inputs of the GPU tests"""
    for mod, dt, n, ms in cc.sweep():
        qad = cc.sweep_qad(oracle, n, dt, mod)
        assert (cc.expected(qad, ms) == "none") == (oracle.detect_center(qad, ms) is None), (mod, dt, n, ms)
    for qad, ms in ((np.full(5000, -4.0, np.float32), None), (np.full(5000, 0.5, np.float32), None), (cc.sweep_qad(oracle, 8193, np.float32, "FSK"), 0)):
        assert cc.expected(qad, ms) == "none" and oracle.detect_center(qad, ms) is None


def test_ties_are_settled_by_numpy_on_the_histogram(oracle):
    """for every 'tie' case estimators.peaks_center on np.histogram's counts and edges is oracle.detect_center: what the hand-out path
    of a flag-3 pass computes from the shipped histogram"""
    from urh_amd import estimators
    ties = 0
    for mod, dt, n, ms in cc.sweep():
        qad = cc.sweep_qad(oracle, n, dt, mod)
        if cc.expected(qad, ms) != "tie":
            continue
        ties += 1
        y, x = cc.histogram(qad, ms)
        # the edges as the result block carries them: e0 + i * delta, np.arange's own fill
        edges = x[0] + np.arange(len(y) + 1, dtype=np.float64) * (x[1] - x[0])
        assert np.array_equal(edges, x), (mod, dt, n, ms)
        got = estimators.peaks_center(y, edges)
        assert got is not None and float(got) == float(oracle.detect_center(qad, ms)), (mod, dt, n, ms)
    assert ties >= 1
