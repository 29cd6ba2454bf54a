"""urhgpu_detect_modulation_dev (urh_amd/csrc/modulation.hip) on the cases of tests/modulation_cases.py, against its float64 reference
-- which tests/test_detect_modulation_host.py pins to the reference's own arithmetic on the same cases --: the label of every message,
and the four variances within modulation_cases.tolerance() in the metric |delta var| / mean(m^2) of the magnitude array m:
T = 256 S = 1.792e-13, S the measured spread between the float64 and the longdouble evaluation of the reference (family F's two filtered
variances: T + 2.8e-12, see the host test).  The bound comes from the reference alone.  Every inequality the reference evaluates has a
relative margin of 1e-3 in every case, so a label that differs is a wrong kernel, not a rounding.

Each test packs its messages into one capture at odd offsets and makes one call per (wavelet_scale, median_filter_order).

What each test is there to catch (a kernel with that change fails it):
  change                                                          tests that fail
  k_md_prepare with a true division or hypot in double            test_variances_* (A-D), test_dropped_samples_*
  k_md_median rounding to float32 the wrong way, or not at all    test_variances_* (A, B; tried: toward zero.  Without the rounding
                                                                  nothing changes while the output array is float32: rounding is monotonic)
  k_md_median with a centred window                               test_variances_* (A, B; B's order 16 on L = 16 cuts every window)
  k_md_wavelet wrapping the upper indices                         test_variances_* (A, B)
  k_md_mag with a wrong 1 / N or a wrong skip                     test_variances_* (A, B: scales 1, 4, 10)
  maximum taken by magnitude                                      test_dropped_samples_and_the_lexicographic_maximum (D)
  compaction off by one at a stretch, wave or tile end            test_dropped_samples_and_the_lexicographic_maximum (C)
  a denormal flushed in md_nonzero / k_md_prepare                 test_dropped_samples_* (C_denormal_*)
  k_md_scan without its carry                                     test_variances_* (F)
  k_md_topk losing a slice's end                                  test_labels_at_the_limits_of_the_last_branch (E)
  dist > 10 or magnitude > 100                                    test_labels_at_the_limits_of_the_last_branch (E)
  stale scratch                                                   test_messages_do_not_see_each_other"""
import ctypes as C

import numpy as np
import pytest

import modulation_cases as M

pytestmark = pytest.mark.gpu

_got = {}


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def pack(msgs):
    """the messages in one capture, each at an odd offset, samples of another message's size between them; (capture, bounds)"""
    parts, bounds, o = [], [], 0
    for k, m in enumerate(msgs):
        gap = 1 if o % 2 == 0 else 2
        parts.append(np.full(gap, complex(0.5 + k, -0.25), np.complex64))
        o += gap
        bounds.append((o, o + len(m)))
        parts.append(m)
        o += len(m)
    parts.append(np.full(3, complex(-7.0, 7.0), np.complex64))
    assert all(a % 2 == 1 for a, _ in bounds)
    return np.concatenate(parts), bounds


def device(pipe, names):
    """(label, variances) of every named case: one call per (scale, order), computed once per case"""
    import torch
    from urh_amd import estimators
    groups = {}
    for n in names:
        if n not in _got:
            c = M.case(n)
            groups.setdefault((c.scale, c.order), []).append(c)
    for (scale, order), cs in groups.items():
        capture, bounds = pack([c.msg for c in cs])
        dev = torch.from_numpy(capture.view(np.float32).reshape(-1, 2)).cuda()
        labels, variances = estimators.detect_modulation_dev(pipe, dev, bounds, wavelet_scale=scale, median_filter_order=order, return_variances=True)
        for c, lab, var in zip(cs, labels, variances):
            _got[c.name] = (lab, var.copy())
    return {n: _got[n] for n in names}


def hold(pipe, names):
    failures = []
    worst = np.zeros(4)
    for n, (lab, var) in device(pipe, names).items():
        r = M.ref(n)
        if r.info["mags"] is None:                          # the reference returns before it computes a variance: NaN exactly there
            ok, m = bool(np.isnan(var).all()), np.zeros(4)
        else:
            m = M.metric(var, r.variances, r)
            ok = bool((m <= M.tolerance(n)).all()) and np.array_equal(np.isnan(var), np.isnan(r.variances))
            worst = np.maximum(worst, m)
        if not ok or lab != r.label:
            failures.append((n, lab, r.label, var.tolist(), r.variances.tolist(), (m / M.T).round(2).tolist()))
    print("largest gaps / T: %s over %d cases" % ((worst / M.T).round(3).tolist(), len(names)))
    assert not failures, ("%d of %d cases; (name, label, want, variances, want, gap / T)" % (len(failures), len(names)), failures[:8])


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "F"])
def test_variances_equal_the_float64_reference(pipe, family):
    assert len(M.names(family)) == M.COUNTS[family]
    hold(pipe, M.names(family))


def test_labels_at_the_limits_of_the_last_branch(pipe):
    assert len(M.names("E")) == M.COUNTS["E"]
    got = device(pipe, M.names("E"))
    for n in M.names("E"):
        r = M.ref(n)
        top = r.info["top"]
        assert got[n][0] == r.label == M.E_EXPECT[n], (n, got[n][0], r.label, "ten greatest (distance, magnitude)",
                                                        [(abs(i - top[0][0]), round(v, 3)) for i, v in top])
    hold(pipe, M.names("E"))


def test_dropped_samples_and_the_lexicographic_maximum(pipe):
    hold(pipe, M.names("C") + M.names("D"))
    got = device(pipe, ["C_drop_3_exactly", "C_drop_4_exactly_ook"])
    assert got["C_drop_3_exactly"][0] == "FSK" and np.isfinite(got["C_drop_3_exactly"][1]).all()
    assert got["C_drop_4_exactly_ook"][0] == "OOK" and np.isnan(got["C_drop_4_exactly_ook"][1]).all()


def test_messages_do_not_see_each_other(pipe):
    import torch
    from urh_amd import estimators
    small = M.case("A_FSK_N256_len257").msg
    order = [small, M.case("A_FSK_N65536_len65537").msg, small, M.case("B_FSK_N16_s4_none").msg, small,
             M.case("C_drop_4_exactly_ook").msg, small, np.zeros(50, np.complex64), small, M.case("A_PSK_N4096_len4097").msg, small,
             np.zeros(0, np.complex64), small]
    capture, bounds = pack(order)
    dev = torch.from_numpy(capture.view(np.float32).reshape(-1, 2)).cuda()
    labels, variances = estimators.detect_modulation_dev(pipe, dev, bounds, return_variances=True)
    capture1, bounds1 = pack([small])
    dev1 = torch.from_numpy(capture1.view(np.float32).reshape(-1, 2)).cuda()
    labels1, variances1 = estimators.detect_modulation_dev(pipe, dev1, bounds1, return_variances=True)
    assert np.isfinite(variances1[0]).all() and labels1[0] == M.ref("A_FSK_N256_len257").label
    for k in range(0, len(order), 2):
        assert labels[k] == labels1[0] and np.array_equal(variances[k].view(np.uint64), variances1[0].view(np.uint64)), (k, variances[k], variances1[0])
    assert labels[1] == M.ref("A_FSK_N65536_len65537").label and labels[9] == M.ref("A_PSK_N4096_len4097").label
    assert [labels[k] for k in (3, 5, 7, 11)] == [None, "OOK", None, None] and np.isnan(variances[[3, 5, 7, 11]]).all()
    r = M.ref("A_FSK_N65536_len65537")
    assert (M.metric(variances[1], r.variances, r) <= M.T).all()


def test_integer_captures(pipe):
    import torch
    from urh_amd import estimators
    import numpy_estimators
    assert len(M.names("G")) == M.COUNTS["G"]
    seen = set()
    for dt in ("int8", "uint8", "int16", "uint16"):
        ns = [n for n in M.names("G") if n.startswith("G_%s_" % dt)]
        raws = []
        for n in ns:
            M.case(n)                                       # builds the integer samples
            raws.append(M.G_RAW[n])
        fill = np.full((1, 2), 3, raws[0].dtype)
        parts, bounds, o = [], [], 0
        for raw in raws:
            gap = 1 if o % 2 == 0 else 2
            parts += [np.repeat(fill, gap, axis=0), raw]
            bounds.append((o + gap, o + gap + len(raw)))
            o += gap + len(raw)
        dev = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts))).cuda()
        labels = estimators.detect_modulation_dev(pipe, dev, bounds)
        for n, raw, lab in zip(ns, raws, labels):
            with np.errstate(all="ignore"):
                want = numpy_estimators.detect_modulation(numpy_estimators._as_complex64(raw))
            assert lab == want == M.ref(n).label, (n, lab, want, M.ref(n).label)
            seen.add(lab)
    assert {"FSK", "ASK", "PSK", "OOK"} <= seen, seen


def test_argument_errors(pipe):
    import torch
    from urh_amd import _lib
    lib = _lib.load()
    n = 300
    dev = torch.from_numpy(M.case("B_FSK_N256_s4_o11").msg.copy().view(np.float32).reshape(-1, 2)).cuda()
    assert dev.shape[0] == n

    def call(ranges, n_msgs, scale=4, order=11):
        ranges = np.ascontiguousarray(ranges, dtype=np.int64)
        labels = np.full(4, -77, np.int32)
        variances = np.full((4, 4), -77.0)
        status = lib.urhgpu_detect_modulation_dev(pipe.ctx.handle, C.c_void_p(dev.data_ptr()), n, C.c_void_p(ranges.ctypes.data), n_msgs, scale, order,
                                                  C.c_void_p(labels.ctypes.data), C.c_void_p(variances.ctypes.data))
        return status, labels, variances

    status, labels, variances = call([[0, n]], 1)
    assert status == _lib.OK and labels[0] != -77 and np.isfinite(variances[0]).all() and (labels[1:] == -77).all() and (variances[1:] == -77.0).all()
    for kwargs in ({"scale": 0}, {"scale": -1}, {"order": 0}, {"order": 17}):
        status, labels, variances = call([[0, n]], 1, **kwargs)
        assert status == _lib.ERR_ARG and (labels == -77).all() and (variances == -77.0).all(), kwargs
    assert call([[0, n]], 1, order=16)[0] == _lib.OK and call([[0, n]], 1, order=1)[0] == _lib.OK
    for bad in ([-1, 10], [20, 10], [0, n + 1]):
        status, labels, variances = call([[0, 100], bad], 2)
        assert status == _lib.ERR_ARG and (labels == -77).all() and (variances == -77.0).all(), bad
    assert call([[0, 100], [n, n]], 2)[0] == _lib.OK                # an empty range at the very end is a range
    status, labels, variances = call([[0, n]], 0)
    assert status == _lib.OK and (labels == -77).all() and (variances == -77.0).all()
    assert call([[0, n]], -1)[0] == _lib.ERR_ARG
