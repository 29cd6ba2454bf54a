"""The host side of the estimate of a session (urh_amd/batch/: estimate_batch, segment_messages_batch; urh_amd/csrc/batch_estimate.hip;
include/urhgpu.h "a batch of captures: message ranges per capture"): the numpy model of the kernel's step-and-run walk against the recorded
reference ranges and the oracle, the factored vote function against the reference's estimates, the code objects' metadata of the new
kernels, and the option checks.  No GPU needed."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import batch_estimate_cases as bc
import model_batch_segments as model
from conftest import ROOT, load_golden


def _all_geometry():
    for dt in bc.GEOMETRY_DTYPES:
        for name, iq, thr in bc.geometry(dt):
            yield f"{np.dtype(dt).name}/{name}", iq, thr
    caps, thr = bc.many()
    for i, iq in enumerate(caps):
        yield f"many/{i}", iq, thr


def test_the_cases_cover_what_they_are_meant_to():
    names = [n for n, _, _ in bc.geometry(np.float32)]
    assert len(names) == len(set(names)) and len(names) >= 24 + 3 + 28 + 4 + 3 + 4
    rec = bc.load_ranges()
    assert len(rec["float32/dip9-at0"]) == 1 and len(rec["float32/dip10-at0"]) == 2           # nine samples do not split, ten do
    assert len(rec["float32/spike9-at54"]) == 0 and len(rec["float32/spike10-at54"]) == 1
    assert len(rec["float32/nan-threshold"]) == 0 and len(rec["float32/equal-threshold"]) == 2
    assert len(rec["int16/full-scale-wraps"]) == 3                                             # the wrapped samples split the first burst
    assert len(rec["float32/gain-low-threshold"]) == 3 and len(rec["float32/gain-high-threshold"]) == 0
    assert rec["float32/opens-in-the-last-10"].tolist() == [[99, 112]] and len(rec["float32/opens-short-of-the-end"]) == 0
    assert sum(len(rec[f"many/{i}"]) for i in range(301)) > 300


def test_model_equals_the_recorded_reference_and_the_oracle(oracle):
    rec = bc.load_ranges()
    n_cases = 0
    for name, iq, thr in _all_geometry():
        got = model.segments(model.above_flags(iq, thr))
        assert np.array_equal(got, rec[name]), name
        want = oracle.segment_messages_from_magnitudes(model.magnitudes(iq), thr) if len(iq) else []
        assert got.tolist() == [list(x) for x in want], name
        assert len(got) <= model.capacity(len(iq)), name                                       # the region's capacity cannot truncate
        n_cases += 1
    assert n_cases == len(rec)


def test_model_walks_random_flags_like_the_reference_loop():
    """the run walk against the sample-by-sample loop of auto_interpretation.pyx:55-111, on random runs around the tolerance"""
    def loop(flags):
        out, n = [], len(flags)
        if n == 0:
            return out
        state, ca, cb, start = (1 if flags[0] else -1), 0, 0, 0
        for i in range(n):
            a = bool(flags[i])
            if state == 1:
                cb = 0 if a else cb + 1
            else:
                ca = ca + 1 if a else 0
            if state == 1 and cb >= 10:
                state = -1
                out.append([start, i - cb])
                cb = ca = 0
            elif state == -1 and ca >= 10:
                state = 1
                start = i - ca
                cb = ca = 0
        if state == 1 and start < n - cb:
            out.append([start, n - cb])
        return out
    rng = np.random.default_rng(11)
    for _ in range(200):
        runs = rng.integers(1, 25, int(rng.integers(1, 40)))
        flags = np.concatenate([np.full(int(r), bool((j + int(runs[0])) & 1)) for j, r in enumerate(runs)])
        assert model.segments(flags).tolist() == loop(flags)


def _per_message_values(np_est, oracle, iq, noise, modulation, segments):
    """(center, tolerance, bit length) per message with tests/numpy_estimators.py and the oracle, as AutoInterpretation.estimate computes them"""
    msgs = oracle.merge_message_segments_for_ook(segments) if modulation == "OOK" else segments
    data = oracle.afp_demod(iq, noise, "ASK" if modulation in ("OOK", "ASK") else modulation, 2)
    cen, tol, bl = [], [], []
    for start, end in msgs:
        c = oracle.detect_center(data[start:end])
        if c is None:
            cen.append(np.nan), tol.append(-1), bl.append(-1)
            continue
        plateaus = oracle.get_plateau_lengths(data[start:end], c, 25)
        t = np_est.estimate_tolerance_from_plateau_lengths(plateaus)
        merged = np_est.merge_plateau_lengths(plateaus, tolerance=t)
        if len(merged) < 2:
            cen.append(c), tol.append(-1 if t is None else t), bl.append(-1)
            continue
        b = np_est.get_bit_length_from_plateau_lengths(merged)
        cen.append(c), tol.append(-1 if t is None else t), bl.append(-1 if b is None else b)
    return np.array(cen, np.float64), np.array(tol, np.int64), np.array(bl, np.int64)


def test_vote_function_reproduces_the_reference_estimates(oracle):
    """estimators.vote_on_messages -- the tail estimate_dev and estimate_batch share -- on per-message values computed WITHOUT the library
    gives tests/golden/estimates.json's dicts for the float32 ASK / FSK golden captures, modulation and noise given"""
    import numpy_estimators as np_est
    from urh_amd.estimators import vote_on_messages
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "estimates.json")))
    checked = 0
    for name in ("ask", "ask_short", "enocean_ask", "fsk", "steckdose"):
        g = load_golden(name)
        iq, mod, noise = np.ascontiguousarray(g["iq"]), str(g["modulation_type"]), float(g["noise_threshold"])
        segments = oracle.segment_messages_from_magnitudes(model.magnitudes(iq), noise)
        for m in ((mod, "OOK") if mod == "ASK" else (mod,)):
            cen, tol, bl = _per_message_values(np_est, oracle, iq, noise, m, segments)
            got = vote_on_messages(m, noise, cen, tol, bl)
            assert bc.same_estimate(got, want[f"{name}|{m}|given"]), (name, m, got)
            checked += 1
    assert checked == 8
    assert vote_on_messages("FSK", 0.1, np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64)) is None
    assert vote_on_messages("FSK", 0.1, [np.nan, 0.5], [3, -1], [-1, 1]) is None


@pytest.fixture(scope="module")
def estimate_asm(tmp_path_factory):
    """batch_estimate.hip compiled to gfx950 assembly (no GPU needed), as tests/test_batch_host.py does for batch.hip"""
    from urh_amd import build
    out = str(tmp_path_factory.mktemp("batch_estimate") / "batch_estimate.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *build.FLAGS, "--offload-device-only", "-S", os.path.join(build.CSRC, "batch_estimate.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def test_segment_kernels_have_no_spills_no_scratch_and_only_the_scans_lds(estimate_asm):
    kernels = re.findall(r"\.name:\s+(\S*k_batch_seg\S+)", estimate_asm)
    assert len(kernels) == 7, kernels                         # five sample types, the scan, the compaction
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        values = [int(v) for v in re.findall(r"\." + key + r":\s+(\d+)", estimate_asm)]
        assert len(values) == 7 and not any(values), (key, values)
    assert "scratch_" not in estimate_asm
    sizes = sorted(int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", estimate_asm))
    assert sizes == [0] * 6 + [2048], sizes          # 256 int64 partial sums of the one-workgroup scan, nothing else


def test_segment_assembly_holds_no_fp32_fma(estimate_asm):
    """no v_fma_f32 / v_fmac_f32 / v_mac_f32: nothing is contracted and the float32 magnitude's root is taken in fp64 and rounded once, so an
    fp32 FMA here could only be x * x + y * y fused into one rounding; the walk finds its runs with find-first-set and a population count"""
    assert not re.search(r"v_fma_f32|v_fmac_f32|v_mac_f32", estimate_asm)
    assert re.search(r"v_sqrt_f64|v_rsq_f64", estimate_asm)
    assert re.search(r"s_ff1_i32_b64", estimate_asm) and re.search(r"s_bcnt1_i32_b64", estimate_asm)


def test_option_checks_need_no_device():
    from urh_amd import _lib, batch
    from urh_amd.pipeline import DevicePipeline
    assert callable(DevicePipeline.estimate_batch) and callable(DevicePipeline.segment_messages_batch)
    noises, mods = batch.check_estimate_options(3, np.float32, None, None)
    assert noises == [None] * 3 and mods == [None] * 3
    noises, mods = batch.check_estimate_options(3, np.int8, 0.5, "OOK")
    assert noises == [0.5] * 3 and mods == ["OOK"] * 3
    noises, mods = batch.check_estimate_options(2, np.int16, [0.1, None], ["FSK", None])
    assert noises == [0.1, None] and mods == ["FSK", None]
    for dt in (np.uint8, np.uint16):               # admitted since tests/test_estimate_routes_gpu.py holds estimate_dev to the reference on them
        assert batch.check_estimate_options(1, dt, None, None) == ([None], [None])
    assert [np.dtype(t).name for t in batch.ESTIMATE_SAMPLE_TYPES] == ["float32", "int8", "int16", "uint8", "uint16"]
    for dt in (np.float64, np.int32, np.uint32, np.complex64):
        with pytest.raises(ValueError, match="float32, int8, uint8, int16 and uint16 captures, not " + np.dtype(dt).name):
            batch.check_estimate_options(1, dt, None, None)
    with pytest.raises(ValueError, match="Unsupported Modulation"):
        batch.check_estimate_options(1, np.float32, None, "QAM")
    with pytest.raises(ValueError, match="one entry per capture"):
        batch.check_estimate_options(3, np.float32, [0.1, 0.2], None)
    with pytest.raises(ValueError, match="one entry per capture"):
        batch.check_estimate_options(3, np.float32, None, ["FSK"])
    lib = _lib.load()
    for n in (0, 1, 19, 20, 21, 20000):
        assert lib.urhgpu_batch_segments_capacity(n) == model.capacity(n) == n // 20 + 1
    # rejected before anything is launched, without a GPU
    assert lib.urhgpu_batch_segments_dev(None, None, _lib.DT_F32, 0, None, None, 0, None, None, None, 0, None, None, None, 0) == _lib.ERR_ARG
    assert lib.urhgpu_batch_demod_dev(None, None, 0, None, None, 0, None, None, None) == _lib.ERR_ARG
    est = batch.BatchEstimates([{"bit_length": 1}, None, None], [None, OverflowError("x"), None], [5, 6, 7])
    assert len(est) == 3 and est[0] == {"bit_length": 1} and est[2] is None and est[-1] is None
    with pytest.raises(OverflowError):
        est[1]
    with pytest.raises(OverflowError):
        list(est)
