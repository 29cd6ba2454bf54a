"""The spectrogram band-pass of the reference's `Filter` (row 6b of SURVEY.md §8a), backed by liburhgpu.so.

Mirrors /root/reference/src/urh/signalprocessing/Filter.py:
    get_filter_length_from_bandwidth :64-67, design_windowed_sinc_lpf :103-119, design_windowed_sinc_bandpass :121-131,
    apply_bandpass_filter :84-101 (np.convolve "same" or the FFT convolution :70-82 -- one centred linear convolution).
The taps are O(1/bw) host arithmetic in float64 / complex128 (the same numpy expressions, hence the same taps); the
O(N * taps) convolution runs on the GPU in fp64 (csrc/bandpass.hip).  numpy's summation order is not defined by the
reference, so the result is compared with a tolerance (tests/test_gpu_parity.py), not bit for bit.
`Filter` / `FilterType` are the reference's three filter types (Filter.py:13-46) on the GPU: the two FIR types through the strict-order FIR
(signal_functions.fir_filter, urhgpu_fir_filter_dev), DC correction -- x - mean(x, axis 0), also what the reference's receive path applies to
every chunk (Device.py:822-823) -- through urhgpu_dc_correct_dev, bit-equal with numpy's expression (csrc/dc_correct.hip).
No CPU fallback: without the library or a GPU every call raises.
"""
import ctypes as C
import math
from enum import Enum

import numpy as np

from . import _lib
from .signal_functions import dtype_code


def get_filter_length_from_bandwidth(bw) -> int:
    """Filter.py:64-67: ceil(4 / bw), forced odd"""
    n = int(math.ceil(4 / bw))
    return n + 1 if n % 2 == 0 else n


def get_bandwidth_from_filter_length(n):
    """Filter.py:60-62"""
    return 4 / n


def design_windowed_sinc_lpf(fc, bw) -> np.ndarray:
    """Filter.py:103-119: Blackman-windowed sinc normalised to unity gain (float64)"""
    n = get_filter_length_from_bandwidth(bw)
    h = np.sinc(2 * fc * (np.arange(n) - (n - 1) / 2.0))
    h = h * np.blackman(n)
    return h / np.sum(h)


def design_windowed_sinc_bandpass(f_low, f_high, bw) -> np.ndarray:
    """Filter.py:121-131: the low-pass shifted to the band centre (complex128)"""
    f_shift = (f_low + f_high) / 2
    f_c = (f_high - f_low) / 2
    n = get_filter_length_from_bandwidth(bw)
    return design_windowed_sinc_lpf(f_c, bw=bw) * np.exp(complex(0, 1) * np.pi * 2 * f_shift * np.arange(0, n, dtype=complex))


def bandpass_taps(f_low, f_high, filter_bw=0.08) -> np.ndarray:
    """The taps apply_bandpass_filter designs (Filter.py:86-92: swap, clip to +-0.5)"""
    if f_low > f_high:
        f_low, f_high = f_high, f_low
    f_low = max(-0.5, min(f_low, 0.5))
    f_high = max(-0.5, min(f_high, 0.5))
    return design_windowed_sinc_bandpass(f_low, f_high, filter_bw)


def _same_geometry(n: int, m: int):
    """(shift, n_out) of the reference's result for a capture of n samples and m taps (Filter.py:96-101)"""
    if n == 0:
        raise ValueError("math domain error")                 # math.log(math.sqrt(0)) in the reference (:96)
    if m < 8 * math.log(math.sqrt(n)):
        return (min(n, m) - 1) // 2, max(n, m)               # np.convolve(data, h, "same")
    # fft_convolve_1d: full[too_much : -too_much] with too_much = (m - 1) // 2
    too_much = (m - 1) // 2
    if too_much == 0:
        return 0, 0                                            # result[0:-0] is empty in the reference
    return too_much, n + m - 1 - 2 * too_much


def apply_bandpass_filter(data, f_low, f_high, filter_bw=0.08, ctx=None) -> np.ndarray:
    """Filter.apply_bandpass_filter (Filter.py:84-101) on host arrays: complex64[N] -> complex128[N]"""
    x = np.ascontiguousarray(np.asarray(data), dtype=np.complex64)
    h = np.ascontiguousarray(bandpass_taps(f_low, f_high, filter_bw), dtype=np.complex128)
    shift, n_out = _same_geometry(len(x), len(h))
    out = np.zeros(n_out, dtype=np.complex128)
    if n_out == 0:
        return out
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.load().urhgpu_bandpass(ctx.handle, C.c_void_p(x.ctypes.data), len(x), C.c_void_p(h.ctypes.data), len(h),
                                           shift, n_out, C.c_void_p(out.ctypes.data)))
    return out


def convolve_dev(pipe, iq, taps, shift, n_out, out_complex64=True, left=None, right=None):
    """out[i] = sum_k taps[k] * X(i + shift - k) on device memory (urhgpu_bandpass_dev).
    iq: complex64 (N,) or float32 (N, 2) tensor on pipe.device; taps: complex128 numpy array or device tensor;
    left / right: optional complex64 tensors that extend the capture (sharded captures) instead of zeros."""
    torch = pipe.torch
    if iq.dtype == torch.complex64:
        iq = torch.view_as_real(iq)
    if iq.dtype != torch.float32 or iq.dim() != 2 or iq.shape[1] != 2 or not iq.is_contiguous():
        raise ValueError("the band-pass takes a contiguous complex64 capture")
    if not torch.is_tensor(taps):
        taps = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.complex128)).to(pipe.device)
    if taps.dtype != torch.complex128 or not taps.is_contiguous():
        raise ValueError("taps must be complex128")

    def edge(t):
        if t is None or t.numel() == 0:
            return None, 0
        if t.dtype == torch.complex64:
            t = torch.view_as_real(t)
        t = t.contiguous()
        return t, t.shape[0]

    left, n_left = edge(left)
    right, n_right = edge(right)
    out = torch.empty(n_out, dtype=torch.complex64 if out_complex64 else torch.complex128, device=pipe.device)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    _lib.check(_lib.load().urhgpu_bandpass_dev(
        pipe.ctx.handle, C.c_void_p(iq.data_ptr()), iq.shape[0], C.c_void_p(taps.data_ptr()), taps.shape[0], shift, n_out,
        C.c_void_p(left.data_ptr()) if left is not None else None, n_left,
        C.c_void_p(right.data_ptr()) if right is not None else None, n_right,
        C.c_void_p(out.data_ptr()), 1 if out_complex64 else 0))
    pipe._bp_keep = (iq, taps, left, right)                   # alive until the next call (asynchronous launch)
    return out


def apply_bandpass_filter_dev(pipe, iq, f_low, f_high, filter_bw=0.08, out_complex64=True):
    """apply_bandpass_filter on a device-resident capture; out_complex64 fuses the cast SignalFrame applies to the result
    (/root/reference/src/urh/controller/widgets/SignalFrame.py:1578-1580)."""
    h = bandpass_taps(f_low, f_high, filter_bw)
    n = iq.shape[0]
    shift, n_out = _same_geometry(n, len(h))
    return convolve_dev(pipe, iq, h, shift, n_out, out_complex64)


# ---- the reference's Filter: moving average, DC correction, custom taps ----------------------------------------------------------------
class FilterType(Enum):
    moving_average = "moving average"
    custom = "custom"
    dc_correction = "DC correction"


_TORCH_CODES = {"torch.int8": _lib.DT_I8, "torch.uint8": _lib.DT_U8, "torch.int16": _lib.DT_I16, "torch.uint16": _lib.DT_U16,
                "torch.float32": _lib.DT_F32}


def dc_correct_dev(pipe, iq, out=None, want_mean=False):
    """out = iq - mean(iq, axis 0) on the device, asynchronous on the current stream (urhgpu_dc_correct_dev).
    iq: contiguous (n, 2) tensor of a sample type (or complex64 (n,)) on pipe.device; out: None (a new tensor), iq itself (in place) or a
    tensor of iq's shape and type that does not overlap it.  want_mean: also return the two means as a device tensor (float32 for a float32
    capture, float64 otherwise)."""
    torch = pipe.torch
    x = torch.view_as_real(iq) if iq.dtype == torch.complex64 else iq
    code = _TORCH_CODES.get(str(x.dtype))
    if code is None:
        raise ValueError("Unsupported dtype")
    if x.dim() != 2 or x.shape[1] != 2 or not x.is_contiguous() or x.device != pipe.device:
        raise ValueError(f"DC correction takes a contiguous (n, 2) capture on {pipe.device}")
    if out is None:
        out = torch.empty_like(iq)
    y = torch.view_as_real(out) if out.dtype == torch.complex64 else out
    if y.shape != x.shape or y.dtype != x.dtype or not y.is_contiguous() or y.device != x.device:
        raise ValueError("out must have the capture's shape, type and device")
    mean = torch.empty(2, dtype=torch.float32 if code == _lib.DT_F32 else torch.float64, device=pipe.device) if want_mean else None
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    _lib.check(_lib.load().urhgpu_dc_correct_dev(pipe.ctx.handle, C.c_void_p(x.data_ptr()), x.shape[0], code, C.c_void_p(y.data_ptr()),
                                                 C.c_void_p(mean.data_ptr()) if want_mean else None))
    return (out, mean) if want_mean else out


def dc_correct(data, ctx=None, want_mean=False):
    """The same on a host array of a sample type, (n, 2) or complex64 (n,) (urhgpu_dc_correct): a new array of the same shape and type."""
    a = np.ascontiguousarray(data)
    x = a.view(np.float32).reshape(-1, 2) if a.dtype == np.complex64 else a
    if x.ndim != 2 or x.shape[1] != 2:
        raise ValueError("DC correction takes an (n, 2) capture")
    code = dtype_code(x.dtype)
    out = np.empty_like(x)
    mean = np.zeros(2, np.float32 if code == _lib.DT_F32 else np.float64)
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.load().urhgpu_dc_correct(ctx.handle, C.c_void_p(x.ctypes.data), x.shape[0], code, C.c_void_p(out.ctypes.data),
                                             C.c_void_p(mean.ctypes.data)))
    out = out.view(np.complex64).reshape(a.shape) if a.dtype == np.complex64 else out
    return (out, mean) if want_mean else out


class Filter:
    """The reference's Filter (Filter.py:13-46): taps and a type.  work(iq) filters a capture -- a device tensor stays on the device, a host
    array goes through the host-pointer entry points."""
    BANDWIDTHS = {"Very Narrow": 0.001, "Narrow": 0.01, "Medium": 0.08, "Wide": 0.1, "Very Wide": 0.42}

    def __init__(self, taps, filter_type: FilterType = FilterType.custom):
        self.filter_type = filter_type
        self.taps = taps

    def work(self, iq, pipe=None, ctx=None):
        """FIR types: the raw sample values as float32 through the FIR with zero history -- complex64 (n,) for a host array, float32 (n, 2)
        for a device tensor.  With empty taps the host route returns what the reference returns (n - 1 zeros; ValueError for an empty
        capture), the device route keeps the capture's length (n zeros).  DC correction: the capture minus its mean in the capture's own sample type, i.e. the reference's float64
        difference after the cast that storing it into an IQArray or the receive buffer applies."""
        if self.filter_type == FilterType.dc_correction:
            if isinstance(iq, np.ndarray):
                return dc_correct(iq, ctx)
            return dc_correct_dev(_need(pipe), iq)
        if self.filter_type not in (FilterType.moving_average, FilterType.custom):
            raise ValueError("Unsupported FilterType")
        if isinstance(iq, np.ndarray):
            from . import signal_functions as sf
            x = iq if iq.dtype == np.complex64 else np.ascontiguousarray(iq, np.float32).reshape(-1, 2).view(np.complex64).reshape(-1)
            return sf.fir_filter(x, np.ascontiguousarray(self.taps, dtype=np.complex64), ctx)
        return fir_filter_dev(_need(pipe), iq, self.taps)

    @staticmethod
    def read_configured_filter_bw() -> float:
        return 0.08


def _need(pipe):
    if pipe is None:
        raise ValueError("a device tensor needs the DevicePipeline it lives on (pipe=...)")
    return pipe


def fir_filter_dev(pipe, iq, taps):
    """Filter.apply_fir_filter on a device capture: the raw sample values as float32 through the strict-order FIR with zero history
    (urhgpu_fir_filter_dev) -> float32 (n, 2).  The result always has the capture's length: empty taps give n zeros, where the reference's
    host function (and signal_functions.fir_filter) gives n - 1."""
    from .iq_array import astype
    torch = pipe.torch
    x = torch.view_as_real(iq) if iq.dtype == torch.complex64 else iq
    x = astype(x.clone(), np.float32, pipe.ctx)                 # a copy: 16-byte aligned whatever slice iq is
    h = np.ascontiguousarray(taps, dtype=np.complex64)
    d_h = torch.from_numpy(h.view(np.float32).copy()).to(pipe.device)
    y = torch.empty_like(x)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    _lib.check(_lib.load().urhgpu_fir_filter_dev(pipe.ctx.handle, C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(d_h.data_ptr()), len(h), None,
                                                 C.c_void_p(y.data_ptr())))
    return y
