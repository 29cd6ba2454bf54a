"""DevicePipeline.dc_correct_batch and iq_to_bits_batch_dc (urh_amd/batch/; include/urhgpu.h "a batch of captures: DC correction per
capture") on the GPU.  Expected values: numpy's own expression per capture (dc_cases.numpy_dc) for the correction, and the existing
single-capture paths -- iq_to_bits, get_protocol_from_signal_dev, estimate_dev -- over numpy-corrected captures for everything built on it;
never the code under test.  The inputs come from tests/batch_dc_cases.py, where tests/test_batch_dc_host.py holds them against the oracle."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import batch_dc_cases as cases
from batch_psk_cases import to_dev
from dc_cases import same_bits

pytestmark = pytest.mark.gpu

IDS = lambda d: np.dtype(d).name          # noqa: E731


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline(0)


def host(t):
    """a device tensor as a numpy array of the same sample type"""
    import torch
    if hasattr(torch, "uint16") and t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def check_captures(iq, starts, means, want, tag):
    got = host(iq)
    assert len(starts) == len(want) + 1 and means.shape == (len(want), 2), tag
    for k, (out, mean) in enumerate(want):
        a = int(starts[k])
        assert int(starts[k + 1]) - a == len(out), (tag, k)
        assert same_bits(got[a:a + len(out)], out), (tag, k, len(out), "output")
        assert same_bits(means[k], mean), (tag, k, len(out), means[k], mean)
    return got


# ---- 1. dc_correct_batch: lengths, sample types, input forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host_list", "device_list", "packed_host", "packed_device"])
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=IDS)
def test_dc_correct_batch_on_the_length_sweep(pipe, dtype, form):
    caps, cat, starts, want = cases.sweep(dtype)
    tag = (np.dtype(dtype).name, form)
    if form == "host_list":
        iq, s, means = pipe.dc_correct_batch(list(caps), want_means=True)
    elif form == "device_list":
        tensors = [to_dev(pipe, c) for c in caps]
        iq, s, means = pipe.dc_correct_batch(tensors, want_means=True)
        for t, c in zip(tensors, caps):
            assert same_bits(host(t), c), (tag, "the caller's tensor was modified")
    elif form == "packed_host":
        iq, s, means = pipe.dc_correct_batch((cat, starts), want_means=True)
    else:
        d_cat = to_dev(pipe, cat)
        iq, s, means = pipe.dc_correct_batch((d_cat, starts), want_means=True)
        assert same_bits(host(d_cat), cat), (tag, "the caller's tensor was modified")
        assert iq.data_ptr() != d_cat.data_ptr()
    got = check_captures(iq, s, means, want, tag)
    if form.startswith("packed"):
        assert np.array_equal(s, starts) and got.shape == cat.shape
    if form == "packed_host":            # corrected in place in its upload: what belongs to no capture still holds the pattern
        a, b = int(starts[0]), int(starts[-1])
        assert same_bits(got[:a], cat[:a]) and same_bits(got[b:], cat[b:]) and len(got) - b == cases.UNUSED_BEHIND
    # the pair is itself the third input form
    again = pipe.dc_correct_batch((iq, s))
    assert again[0].shape == iq.shape and np.array_equal(again[1], s)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=IDS)
def test_no_capture_and_empty_captures(pipe, dtype):
    iq, s, means = pipe.dc_correct_batch([], want_means=True)
    assert iq.shape == (0, 2) and list(s) == [0] and means.shape == (0, 2)
    empty = np.zeros((0, 2), dtype)
    for captures in ([empty, empty, empty], [to_dev(pipe, empty)] * 3, (empty, [0, 0, 0, 0])):
        iq, s, means = pipe.dc_correct_batch(captures, want_means=True)
        assert iq.shape == (0, 2) and list(s) == [0, 0, 0, 0] and means.shape == (3, 2) and np.isnan(means).all()
        assert means.dtype == (np.float32 if dtype == np.float32 else np.float64)


# ---- 2. values -------------------------------------------------------------------------------------------------------------------------------
def test_float32_values(pipe):
    """NaN and infinities in a sum, overflow, denormals, negative zero, ties with even and odd k, sums that cross binades -- side by side in
    one batch"""
    names, caps, want = cases.f32_values()
    iq, s, means = pipe.dc_correct_batch(list(caps), want_means=True)
    for k, name in enumerate(names):
        print(name, "mean", means[k], "numpy", want[k][1])
    got = check_captures(iq, s, means, want, "float32 values")
    k = names.index(f"neg_zero:{cases.F32_N}")
    assert np.signbit(got[int(s[k]):int(s[k + 1])]).all() and not np.signbit(means[k]).any()


@pytest.mark.parametrize("name", ["int8_alternating", "uint8_around_128", "uint16_wrap", "int16_extremes"])
def test_integer_values(pipe, name):
    caps, want = cases.int_values(name)
    for captures in (list(caps), [to_dev(pipe, c) for c in caps]):
        iq, s, means = pipe.dc_correct_batch(captures, want_means=True)
        check_captures(iq, s, means, want, name)


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=IDS)
def test_c_abi_in_place_out_of_place_and_refusals(pipe, dtype):
    import torch
    from urh_amd import _lib, batch
    from urh_amd.signal_functions import dtype_code
    caps, cat, starts, want = cases.sweep(dtype)
    lib, h, k, total = _lib.load(), pipe.ctx.handle, len(caps), len(cat)
    plan, _, _ = batch.batch_plan(np.diff(starts), cases.demod_set("fsk")[1].to_c(dtype))
    d_meta = torch.from_numpy(np.concatenate([starts, plan]).astype(np.int64)).to(pipe.device)
    d_start, d_plan = C.c_void_p(d_meta.data_ptr()), C.c_void_p(d_meta.data_ptr() + 8 * (k + 1))
    d_in, d_out = to_dev(pipe, cat), to_dev(pipe, cases.sentinel(dtype, total))
    d_mean = torch.zeros(2 * k, dtype=torch.float32 if dtype == np.float32 else torch.float64, device=pipe.device)
    code, item = dtype_code(np.dtype(dtype)), 2 * np.dtype(dtype).itemsize
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)

    def call(src, dst, mean=d_mean, dt=code, n=k):
        return lib.urhgpu_batch_dc_correct_dev(h, C.c_void_p(src), total, dt, d_start, d_plan, n, C.c_void_p(dst), C.c_void_p(mean.data_ptr()) if mean is not None else None)
    a, b = d_in.data_ptr(), d_out.data_ptr()
    assert call(a, b, dt=7) == _lib.ERR_DTYPE
    assert call(a, a + 16) == _lib.ERR_ARG and call(a + 16, a) == _lib.ERR_ARG               # overlap
    assert call(a + item // 2, b) == _lib.ERR_ARG and call(a, b + item // 2) == _lib.ERR_ARG   # half a sample
    assert call(a, b, n=-1) == _lib.ERR_ARG
    assert call(a, b, n=0) == _lib.OK
    torch.cuda.synchronize()
    assert same_bits(host(d_out), cases.sentinel(dtype, total)) and not d_mean.any()         # k == 0 launched nothing
    # out of place, with and without the means; then in place
    assert call(a, b, mean=None) == _lib.OK
    first = host(d_out).copy()
    assert call(a, b) == _lib.OK
    means = d_mean.cpu().numpy().reshape(k, 2)
    assert same_bits(host(d_in), cat), "the input was modified"
    out = check_captures(d_out, starts, means, want, "out of place")
    assert same_bits(out, first)
    lo, hi = int(starts[0]), int(starts[-1])
    assert same_bits(out[:lo], cases.sentinel(dtype, total)[:lo]) and same_bits(out[hi:], cases.sentinel(dtype, total)[hi:]), "written outside the captures"
    assert call(a, a) == _lib.OK
    inplace = host(d_in)
    assert same_bits(inplace[lo:hi], out[lo:hi]) and same_bits(inplace[:lo], cat[:lo]) and same_bits(inplace[hi:], cat[hi:])
    assert same_bits(d_mean.cpu().numpy().reshape(k, 2), means)


# ---- 4. iq_to_bits_batch_dc against the pass over numpy-corrected captures ---------------------------------------------------------------------
def got_of(h):
    return [np.array(x) for x in (h.ppseq(), h.bits(), h.msg_off, h.pauses, h.bit_sample_pos(), h.pos_offsets())]


def kept_of(res, options):
    """what a batch handed out, copied out of the pipeline's buffers"""
    out = []
    for i in range(len(res)):
        assert res[i].truncated == 0 and res[i].seq == i, i
        out.append({"got": got_of(res[i]), "qad": res.qad(i).cpu().numpy().copy(), "n": res[i].n_samples,
                    "noise": (res.noise[i], res.noise_flags[i]) if options.get("auto_noise") else None,
                    "center": (res.centers[i], res.center_flags[i]) if options.get("auto_center") else None,
                    "rec": np.array(res[i].records) if options.get("msg_records") else None})
    return out


def same_kept(a, b, tag):
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(u, v) for u, v in zip(x["got"], y["got"])), (tag, i)
        assert x["qad"].tobytes() == y["qad"].tobytes() and x["n"] == y["n"] and x["noise"] == y["noise"] and x["center"] == y["center"], (tag, i)
        assert (x["rec"] is None and y["rec"] is None) or x["rec"].tobytes() == y["rec"].tobytes(), (tag, i)


def same_as_the_pass(pipe, kept, corrected, p, options, tag):
    """entry k of `kept` against iq_to_bits on the numpy-corrected capture k alone"""
    for i, x in enumerate(corrected):
        one = pipe.iq_to_bits(to_dev(pipe, x), replace(p, write_bit_sample_pos=True), want_qad=True, cap_rows=len(x) // (p.tolerance + 1) + 2, **options)
        h = one.host(pool={})
        k = kept[i]
        assert h.n_samples == k["n"], (tag, i)
        for u, v in zip(k["got"], got_of(h)):
            assert np.array_equal(u, v), (tag, i)
        assert len(k["got"][0]) > 10, (tag, i)
        assert k["qad"].view(np.uint32).tobytes() == one.qad.cpu().numpy()[:len(k["qad"])].view(np.uint32).tobytes(), (tag, i, "qad")
        if options.get("auto_noise"):
            assert one.noise_flag == k["noise"][1] and float(one.noise_threshold).hex() == float(k["noise"][0]).hex(), (tag, i)
        if options.get("auto_center"):
            assert (one.center, one.center_flag) == k["center"], (tag, i, one.center, k["center"])
        if options.get("msg_records"):
            assert np.array(one.records).tobytes() == k["rec"].tobytes(), (tag, i, "records")


def matching_batch(pipe, captures, p, options, **kw):
    """the batch iq_to_bits_batch_dc runs behind the correction, called on its own"""
    from urh_amd.batch import is_psk
    o = cases.batch_options(options)
    if is_psk(p):
        return pipe.iq_to_bits_batch_psk(captures, p, auto_center=bool(options.get("auto_center")), **o, **kw)
    if "message_length_divisor" in o:
        return pipe.iq_to_bits_batch_records(captures, p, auto_center=bool(options.get("auto_center")), **o, **kw)
    if options.get("auto_center"):
        return pipe.iq_to_bits_batch_center(captures, p, auto_noise=o["auto_noise"], **kw)
    if o["auto_noise"]:
        return pipe.iq_to_bits_batch_auto(captures, p, **kw)
    return pipe.iq_to_bits_batch(captures, p, **kw)


def dc_batch(pipe, captures, p, options, **kw):
    return pipe.iq_to_bits_batch_dc(captures, p, auto_center=bool(options.get("auto_center")), want_qad=True, **cases.batch_options(options), **kw)


def set_of(kind):
    caps, p, dtype, options, corrected = cases.demod_set(kind.split("+")[0])
    if kind.endswith("+auto_center"):
        options = dict(options, auto_center=True)
    return caps, p, dtype, options, corrected


@pytest.mark.parametrize("kind", [*cases.SETS, "fsk+auto_center"])
def test_iq_to_bits_batch_dc_equals_the_pass_over_corrected_captures(pipe, kind):
    from urh_amd.batch import launch_counts
    caps, p, dtype, options, corrected = set_of(kind)
    tensors = [to_dev(pipe, c) for c in caps]
    l0 = launch_counts(pipe)
    res = dc_batch(pipe, tensors, p, options, cap_rows="bound")
    l1 = launch_counts(pipe)
    kept = kept_of(res, options)
    means = np.array(res.means)
    matching_batch(pipe, [to_dev(pipe, x) for x in corrected], p, options, want_qad=True, cap_rows="bound")
    l2 = launch_counts(pipe)
    assert l1[0] - l0[0] == l2[0] - l1[0] + 2, (kind, l0, l1, l2)                 # two launches more, whatever K is
    for t, c in zip(tensors, caps):
        assert same_bits(host(t), c), "the caller's capture was modified"
    for i, c in enumerate(caps):
        assert same_bits(means[i], cases.numpy_dc(c)[1]), (kind, i)
    same_as_the_pass(pipe, kept, corrected, p, options, kind)
    # the other two input forms
    same_kept(kept_of(dc_batch(pipe, list(caps), p, options, cap_rows="bound"), options), kept, (kind, "host list"))
    cat, starts = cases.pack(caps, dtype)
    d_cat = to_dev(pipe, cat)
    same_kept(kept_of(dc_batch(pipe, (d_cat, starts), p, options, cap_rows="bound"), options), kept, (kind, "packed"))
    assert same_bits(host(d_cat), cat), "the caller's buffer was modified"


# ---- 5. routing by length ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fsk", "ask_i16_auto_noise_records"])
def test_long_captures_go_through_the_pass_with_its_own_correction(pipe, kind):
    caps, p, dtype, options, corrected = set_of(kind)
    assert 0 < sum(len(c) >= 20_000 for c in caps) < len(caps)
    res = dc_batch(pipe, list(caps), p, options, cap_rows=None, long_from=20_000)
    kept, means = kept_of(res, options), np.array(res.means)
    for i, c in enumerate(caps):
        assert same_bits(means[i], cases.numpy_dc(c)[1]), (kind, i)
    same_as_the_pass(pipe, kept, corrected, p, options, (kind, "long_from"))


# ---- 6. truncation and retry -------------------------------------------------------------------------------------------------------------------
def test_a_truncated_capture_is_corrected_and_run_again(pipe):
    caps, p, dtype, options, corrected = set_of("ask_i16_auto_noise_records")
    whole = kept_of(dc_batch(pipe, list(caps), p, options, cap_rows="bound"), options)
    res = dc_batch(pipe, list(caps), p, options, cap_rows=16)
    cut = res.truncated
    assert cut, "no capture was truncated: the case shows nothing"
    for k in cut:
        h = res.retry(k)
        assert h.truncated == 0
        assert all(np.array_equal(u, v) for u, v in zip(got_of(h), whole[k]["got"])), k
        assert np.array(h.records).tobytes() == whole[k]["rec"].tobytes() and res.qad(k).cpu().numpy().tobytes() == whole[k]["qad"].tobytes(), k
    assert res.truncated == []


# ---- 7. the session's messages -----------------------------------------------------------------------------------------------------------------
def test_get_protocols_from_signals_dev_with_dc_correction(pipe):
    from urh_amd import protocol
    caps, p, dtype, options, corrected = set_of("ask_i16_auto_noise_records")
    got = protocol.get_protocols_from_signals_dev(pipe, list(caps), p, 4, sample_rate=2e6, timestamps=[3.5] * len(caps), dc_correction=True)
    got = [[(list(m.plain_bits), m.pause, list(m.bit_sample_pos), np.float64(m.rssi).tobytes(), m.timestamp) for m in msgs] for msgs in got]
    assert len(got) == len(caps)
    for i, x in enumerate(corrected):
        want = protocol.get_protocol_from_signal_dev(pipe, to_dev(pipe, x), p, 4, sample_rate=2e6, timestamp=3.5)
        assert len(want) > 0 and len(got[i]) == len(want), i
        for a, b in zip(got[i], want):
            assert a == (list(b.plain_bits), b.pause, list(b.bit_sample_pos), np.float64(b.rssi).tobytes(), b.timestamp), i


# ---- 8. composition ----------------------------------------------------------------------------------------------------------------------------
def test_the_corrected_pair_feeds_the_other_batch_methods(pipe):
    from urh_amd import estimators as E
    caps, p, dtype, options, corrected = set_of("fsk")
    pair = pipe.dc_correct_batch(list(caps))
    est = pipe.estimate_batch(pair)
    noise = pipe.detect_noise_levels(pair)
    assert len(est) == len(caps) == len(noise)
    for i, x in enumerate(corrected):
        assert est[i] == E.estimate_dev(pipe, to_dev(pipe, x)), i
        assert est[i] is not None and noise[i] == E.detect_noise_level_dev(pipe, to_dev(pipe, x)), i
    kept = kept_of(pipe.iq_to_bits_batch(pair, p, want_qad=True, cap_rows="bound"), {})
    same_as_the_pass(pipe, kept, corrected, p, {}, "iq_to_bits_batch(dc_correct_batch(...))")
