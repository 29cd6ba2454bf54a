"""The input forms of a batch, the routing by length, and options given once or per capture."""
from collections import namedtuple

import numpy as np

# a capture of this many samples or more goes through an ordinary pass: the capture length at which a batch's wavefront per capture stops
# beating a pipelined stream's pass per capture -- measured: B / A = 1.39 at 131 072 samples, 1.02 and 0.98 at 196 608 (two runs), 0.98 at 262 144
# (tools/batch_probe.py, profiles/batch_probe.txt; DESIGN.md 7.7e has the table).  PSK keeps it: no measured set has the stream ahead of
# iq_to_bits_batch_psk at or below it -- B / A = 22.7 for 341 captures of 196 608 samples (tools/batch_psk_probe.py,
# profiles/batch_psk_probe.txt)
LONG_FROM_DEFAULT = 196_608


def route(lengths, long_from=None):
    """(indices of the captures the batch takes, indices of those that go through an ordinary pass: long_from samples or more)"""
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.nonzero(lengths < long_from)[0], np.nonzero(lengths >= long_from)[0]


def per_capture(value, k, name, check=None):
    """an option given once for all captures or once per capture, as a list of k entries (host arithmetic)"""
    if value is None or isinstance(value, (str, int, float, np.floating, np.integer)):
        out = [value] * k
    else:
        out = list(value)
        if len(out) != k:
            raise ValueError(f"{name} holds one entry per capture ({k}), or is one value for all")
    if check is not None:
        for v in out:
            check(v)
    return out


def back_to_back(lengths):
    """int64[K + 1]: where captures of these lengths start when they lie back to back from sample 0"""
    starts = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=starts[1:])
    return starts


def _as_rows(a):
    """a capture as a contiguous (N, 2) numpy array of one of the five sample types"""
    a = np.asarray(a)
    if a.dtype == np.complex64 and a.ndim == 1:
        a = a.view(np.float32).reshape(-1, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("a capture must be an (N, 2) array (or complex64 (N,))")
    if a.dtype not in (np.int8, np.uint8, np.int16, np.uint16, np.float32):
        raise ValueError("Unsupported dtype")
    return np.ascontiguousarray(a)


class BatchInput(namedtuple("BatchInput", "caps on_device packed cat starts npdt lengths")):
    """the captures of a batch as given: numpy arrays or device tensors, (N, 2) each; packed: given as (iq_cat, starts), which cat and starts hold"""

    def tensor(self, pipe, i):
        """capture i alone as a contiguous device tensor"""
        c = self.caps[i]
        return (c if self.on_device else pipe.torch.from_numpy(c).to(pipe.device)).contiguous()

    def device_cat(self, pipe, idx=None, keep_geometry=False):
        """the captures idx (None: all) of a device input: (a contiguous (total, 2) device tensor, their starts in it -- None: back to back from
        sample 0).  A packed tensor of which all captures are taken is read where it lies when it is contiguous; otherwise the captures are
        gathered with one torch.cat -- or, with keep_geometry, the packed tensor is copied whole and keeps its starts."""
        torch = pipe.torch
        whole = idx is None or len(idx) == len(self.caps)
        if self.packed and whole and (keep_geometry or self.cat.is_contiguous()):
            return self.cat.contiguous(), self.starts
        caps = self.caps if idx is None else [self.caps[i] for i in idx]
        if caps:
            return torch.cat(caps).contiguous(), None
        from ..iq_array import _torch_dtype_for
        return torch.empty((0, 2), dtype=_torch_dtype_for(self.npdt), device=pipe.device), None


def _batch_input(pipe, captures) -> BatchInput:
    """the three input forms of a batch -- a list of (N, 2) / complex64 numpy arrays, a list of device tensors, (iq_cat, starts) with a numpy
    array or a device tensor"""
    torch = pipe.torch
    from ..pipeline import _torch_dtype
    cat = starts_in = None
    packed = isinstance(captures, tuple) and len(captures) == 2 and not isinstance(captures[0], (list, tuple))
    if packed:
        cat, starts_in = captures
        starts_in = np.asarray(starts_in, dtype=np.int64)
        if starts_in.ndim != 1 or starts_in.size < 1 or (np.diff(starts_in) < 0).any() or starts_in[0] < 0 or starts_in[-1] > len(cat):
            raise ValueError("starts must be K + 1 ascending sample indices inside iq_cat")
        on_device = torch.is_tensor(cat)
        if on_device and cat.dtype == torch.complex64:
            cat = torch.view_as_real(cat)
        if not on_device:
            cat = _as_rows(cat)
        caps = [cat[int(a):int(b)] for a, b in zip(starts_in[:-1], starts_in[1:])]
    else:
        caps = list(captures)
        on_device = bool(caps) and torch.is_tensor(caps[0])
        if on_device:
            caps = [torch.view_as_real(c) if c.dtype == torch.complex64 else c for c in caps]
        else:
            caps = [_as_rows(c) for c in caps]
    if on_device:
        for c in caps:
            if c.dim() != 2 or c.shape[1] != 2:
                raise ValueError("IQ must be (N, 2) tensors")
    dts = {(_torch_dtype(c) if on_device else c.dtype) for c in caps}
    if len(dts) > 1:
        raise ValueError("the captures of a batch share one sample type")
    npdt = np.dtype(dts.pop()) if dts else np.dtype(np.float32)
    return BatchInput(caps, on_device, packed, cat, starts_in, npdt, [int(c.shape[0]) for c in caps])


def _qad_batch_input(pipe, captures):
    """(qad_cat, starts) as a contiguous float32 device tensor and K + 1 ascending sample indices inside it"""
    torch = pipe.torch
    if not (isinstance(captures, tuple) and len(captures) == 2):
        raise ValueError("the demodulated captures are given as (qad_cat, starts)")
    cat, starts = captures
    starts = np.asarray(starts, dtype=np.int64)
    if not torch.is_tensor(cat):
        cat = torch.from_numpy(np.ascontiguousarray(cat, dtype=np.float32)).to(pipe.device)
    if cat.dim() != 1 or cat.dtype != torch.float32:
        raise ValueError("qad_cat must be a float32 vector")
    if starts.ndim != 1 or starts.size < 1 or (np.diff(starts) < 0).any() or starts[0] < 0 or starts[-1] > cat.shape[0]:
        raise ValueError("starts must be K + 1 ascending sample indices inside qad_cat")
    return cat.contiguous(), starts
