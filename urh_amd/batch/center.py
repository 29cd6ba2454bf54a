"""A center per capture: the chain's device memory, the fetch of its result blocks, what the host settles, and the chain alone."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib
from .inputs import _qad_batch_input
from .staging import _pinned, order_params

# counts the tie pool of a batch holds per capture: a demodulated capture's histogram has a few dozen bins (medians of 45 - 81 on the gain
# sweep of tests/batch_center_cases.py), and a tied capture that does not fit goes through the single-range estimator
TIE_POOL_COUNTS_PER_CAPTURE = 128


def batch_center_plan(lengths, total, max_bins):
    """urhgpu_batch_center_plan: (scratch bytes, groups, captures per group) of the center chain over K captures in a buffer of `total`
    samples (None: the sum of the lengths) with a pool of max_bins bins per capture.  Host arithmetic: works without a GPU."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    out = (C.c_int64(0), C.c_int64(0), C.c_int64(0))
    _lib.check(_lib.load().urhgpu_batch_center_plan(lengths.ctypes.data_as(C.c_void_p), int(lengths.size), -1 if total is None else int(total), int(max_bins),
                                                    C.byref(out[0]), C.byref(out[1]), C.byref(out[2])))
    return tuple(int(x.value) for x in out)


def center_thresholds(p, centers):
    """float32 [K][order - 1]: urhgpu_get_center_thresholds' arithmetic -- fp32 multiply, then add / sub -- on (float)center per capture,
    p.center where the entry is None: what k_batch_center_publish writes on the device"""
    order = 1 << p.bits_per_symbol
    half = order // 2
    c = np.array([p.center if x is None else x for x in centers], dtype=np.float64).astype(np.float32).reshape(-1, 1)
    i = np.arange(order - 1)
    below = (i < half).reshape(1, -1)
    mult = np.where(i < half, half - (i + 1), i + 1 - half).astype(np.float32).reshape(1, -1)
    step = mult * np.float32(p.center_spacing)
    return np.ascontiguousarray(np.where(below, c - step, c + step).astype(np.float32))


# the device memory of the chain's scratch and outputs over K captures, with their sizes
CenterBuffers = namedtuple("CenterBuffers", "k scratch scratch_bytes thr cap_thr res tie cap_tie")


def _center_buffers(pipe, k, total, order, cap_tie, max_bins=None) -> CenterBuffers:
    torch = pipe.torch
    max_bins = int(_lib.load().urhgpu_center_hist_cap(pipe.ctx.handle)) if max_bins is None else max_bins
    scratch_bytes, _, _ = batch_center_plan(np.zeros(k, np.int64), total, max_bins)
    cap_tie = TIE_POOL_COUNTS_PER_CAPTURE * max(k, 1) if cap_tie is None else int(cap_tie)
    scratch = pipe._buf("batch:center_scratch", (max(scratch_bytes, 256),), torch.uint8)
    cap_thr = max(k * (order - 1), 1)
    thr = pipe._buf("batch:thr", (cap_thr,), torch.float32)
    res = pipe._buf("batch:center_res", (C.sizeof(_lib.BatchCenterResult) * (k + 1),), torch.uint8)
    tie = pipe._buf("batch:tie", (max(cap_tie, 1),), torch.int32)
    return CenterBuffers(k, scratch, scratch_bytes, thr, cap_thr, res, tie, cap_tie)


def _settle_centers(pipe, blocks, counts, k, qad, starts, n_of, max_size, skip=()):
    """(centers, flags as the device reported them, indices whose center the HOST settled to a value) for the K result blocks: flag 1 -- the
    device's center; 0 -- None; 3 with the histogram in the tie pool -- pipeline.decide_center on the shipped counts; 2, and a tie that did
    not fit the pool -- the single-range estimator on the capture's slice of qad.  skip: captures that are not handed out (noise flag 0)."""
    from ..pipeline import decide_center
    centers, flags, settled = [None] * k, [0] * k, []
    for i in range(k):
        r = blocks[i].r
        flag = flags[i] = int(r.flag)
        if i in skip or flag == 0:
            continue
        if flag == 1:
            centers[i] = float(r.center)
            continue
        nb = int(r.n_bins)
        shipped = counts[int(blocks[i].counts_off):int(blocks[i].counts_off) + nb] if (flag == 3 and nb > 0 and int(r.n_counts) == nb) else None
        s0 = int(starts[i])
        centers[i] = decide_center(flag, r.center, shipped, r.e0, r.delta, pipe, None if shipped is not None else qad[s0:s0 + n_of(i)], max_size)
        if centers[i] is not None:
            settled.append(i)
    return centers, flags, settled


def fetch_and_settle(pipe, pool, bufs, qad, starts, n_of, max_size, skip=()):
    """urhgpu_batch_center_fetch -- the K result blocks and the used part of the tie pool, two copies at most --, then _settle_centers (looked up
    in this module when called: tools/batch_center_probe.py times it here)"""
    torch, k, cap_tie = pipe.torch, bufs.k, bufs.cap_tie
    h_res = _pinned(torch, pool, "batch_center_res", C.sizeof(_lib.BatchCenterResult) * (k + 1))
    h_tie = _pinned(torch, pool, "batch_tie", 4 * max(cap_tie, 1))
    used = C.c_int64(0)
    _lib.check(_lib.load().urhgpu_batch_center_fetch(pipe.ctx.handle, C.c_void_p(bufs.res.data_ptr()), k, C.c_void_p(bufs.tie.data_ptr()), cap_tie,
                                                     C.c_void_p(h_res.data_ptr()), C.c_void_p(h_tie.data_ptr()), cap_tie, C.byref(used)))
    blocks = (_lib.BatchCenterResult * (k + 1)).from_address(h_res.data_ptr())
    counts = h_tie.numpy()[:4 * int(used.value)].view(np.uint32)
    return _settle_centers(pipe, blocks, counts, k, qad, starts, n_of, max_size, skip)


def detect_centers(pipe, captures, max_size=None, return_flags=False, _cap_tie=None, _pool=None):
    """DevicePipeline.detect_centers (see there)"""
    torch = pipe.torch
    qad, starts = _qad_batch_input(pipe, captures)
    k = len(starts) - 1
    pool = pipe._pinned if _pool is None else _pool
    cp = order_params().to_c(np.float32)                   # (the chain reads the demodulated signal alone)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    d_start = pipe._buf("batch:center_starts", (k + 1,), torch.int64)
    d_start.copy_(torch.from_numpy(starts), non_blocking=False)
    total = int(qad.shape[0])
    bufs = _center_buffers(pipe, k, total, 2, _cap_tie)
    _lib.check(_lib.load().urhgpu_batch_center_dev(pipe.ctx.handle, C.c_void_p(qad.data_ptr()), total, C.c_void_p(d_start.data_ptr()), k, C.byref(cp),
                                                   -1 if max_size is None else int(max_size), None, C.c_void_p(bufs.scratch.data_ptr()), bufs.scratch_bytes,
                                                   None, 0, C.c_void_p(bufs.res.data_ptr()), k + 1, C.c_void_p(bufs.tie.data_ptr()), bufs.cap_tie))
    lengths = np.diff(starts)
    centers, flags, _ = fetch_and_settle(pipe, pool, bufs, qad, starts, lambda i: int(lengths[i]), max_size)
    return (centers, flags) if return_flags else centers
