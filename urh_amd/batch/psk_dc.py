"""The Costas loop per capture (urh_amd/csrc/batch_psk.hip) and the DC correction per capture (urh_amd/csrc/batch_dc.hip), which return without waiting."""
import ctypes as C

import numpy as np

from .. import _lib
from .inputs import _batch_input, back_to_back
from .options import as_fsk, check_batch_psk_options
from .staging import _idle_stage, _stage_in_flight, batch_plan, captures_at, order_params, upload, write_noise_blocks


def costas_demod_batch(pipe, captures, p, noise=None, _pool=None):
    """DevicePipeline.costas_demod_batch (see there)"""
    check_batch_psk_options(p)
    torch = pipe.torch
    pool = pipe._pinned if _pool is None else _pool
    given = _batch_input(pipe, captures)
    k = len(given.lengths)
    if noise is not None and len(noise) != k:
        raise ValueError("noise holds one threshold per capture (or is None: p.noise_threshold for all)")
    cp = p.to_c(given.npdt)
    plan, _, _ = batch_plan(given.lengths, as_fsk(p).to_c(given.npdt))
    starts = given.starts if given.packed else back_to_back(given.lengths)
    if given.on_device:
        iq, _ = given.device_cat(pipe, keep_geometry=True)
        total = int(iq.shape[0])
    else:                                                  # (uploaded as bytes: every sample type the same way)
        host = given.cat if given.packed else (np.concatenate(given.caps) if given.caps else np.zeros((0, 2), given.npdt))
        total = int(host.shape[0])
        iq = torch.from_numpy(np.ascontiguousarray(host).reshape(-1).view(np.uint8)).to(pipe.device)
    block = C.sizeof(_lib.NoiseResult)

    def fill(payload):                                     # a result block per capture as k_batch_noise leaves it for flag 1
        payload[:] = 0
        write_noise_blocks(payload.ctypes.data, noise)
    # nothing below waits for the stream: the staging buffer is one no earlier call's upload is still reading (_idle_stage; with room for the
    # blocks whether they are given or not, so that the next call finds it long enough), the device buffer of this call alone (the launch
    # before may still read its own)
    up = upload(pipe, lambda n: _idle_stage(torch, pool, "batch_costas_stages", n if noise is not None else n + block * k),
                lambda n: torch.empty(max(n, 8), dtype=torch.uint8, device=pipe.device), starts, plan,
                payload_bytes=block * k if noise is not None else 0, fill=fill if noise is not None else None)
    _stage_in_flight(torch, pool, "batch_costas_stages", up.stage, up.stream)
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device)
    _lib.check(_lib.load().urhgpu_batch_costas_dev(pipe.ctx.handle, C.c_void_p(iq.data_ptr()), total, C.c_void_p(up.d_start), C.c_void_p(up.d_plan), k, C.byref(cp),
                                                   C.c_void_p(up.d_payload) if noise is not None else None, C.c_void_p(qad.data_ptr())))
    return qad[:total], starts                             # (queued on torch's current stream: the samples' memory is not reused before the launch has run)


def _dc_correct(pipe, pool, given, idx=None):
    """urhgpu_batch_dc_correct_dev on the captures idx (None: all) of a batch's input; a packed buffer of which all captures are taken is
    taken whole, with its geometry: one upload -- starts, plan and, for host captures, every sample --, two launches, nothing waited for.
    Host captures are corrected in place in their upload, a concatenation made here in place too; a caller's device tensor is read and the
    result written into a buffer of the same geometry.  Returns (iq_cat (total, 2) on the device, starts, the means as a device tensor of
    2 K float32 / float64)."""
    from ..iq_array import _torch_dtype_for
    from ..signal_functions import dtype_code
    torch, npdt = pipe.torch, np.dtype(given.npdt)
    caps = given.caps if idx is None else [given.caps[i] for i in idx]
    lengths = np.asarray(given.lengths if idx is None else [given.lengths[i] for i in idx], dtype=np.int64).reshape(-1)
    k = len(caps)
    plan, _, _ = batch_plan(lengths, order_params().to_c(npdt))              # (of the plan only the launch order is read)
    whole = given.packed and k == len(given.caps)
    starts, total = (given.starts, int(len(given.cat))) if whole else (back_to_back(lengths), int(lengths.sum()))
    item = 2 * npdt.itemsize
    if given.on_device:
        fill = None
    elif whole:
        def fill(payload):
            payload[:] = given.cat.reshape(-1).view(np.uint8)
    else:
        fill = captures_at(caps, starts, item)
    # nothing below waits for the stream: the staging buffer is one no earlier call's upload is still reading (_idle_stage), the device buffer
    # of this call alone (the result of a host batch is a view of it)
    up = upload(pipe, lambda n: _idle_stage(torch, pool, "batch_dc_stages", n), lambda n: torch.empty(n, dtype=torch.uint8, device=pipe.device), starts, plan,
                payload_bytes=0 if given.on_device else total * item, fill=fill)
    _stage_in_flight(torch, pool, "batch_dc_stages", up.stage, up.stream)
    if not given.on_device:
        src = out = up.dev_in[up.meta_bytes:up.in_bytes].view(_torch_dtype_for(npdt)).reshape(total, 2)
    else:
        src, _ = given.device_cat(pipe, idx, keep_geometry=True)
        mine = not (whole and given.cat.is_contiguous())                         # a tensor made here may be corrected where it lies
        if src.data_ptr() % 16:                                                  # (a view that starts off a 16-byte boundary)
            src, mine = src.clone(), True
        out = src if mine else torch.empty_like(src)
    d_mean = torch.empty(max(2 * k, 1), dtype=torch.float32 if npdt == np.float32 else torch.float64, device=pipe.device)
    _lib.check(_lib.load().urhgpu_batch_dc_correct_dev(pipe.ctx.handle, C.c_void_p(src.data_ptr()), total, dtype_code(npdt), C.c_void_p(up.d_start),
                                                       C.c_void_p(up.d_plan), k, C.c_void_p(out.data_ptr()), C.c_void_p(d_mean.data_ptr())))
    return out, starts, d_mean[:2 * k]     # (queued on torch's current stream: no memory of this call is reused before the launches have run)


def dc_correct_batch(pipe, captures, want_means=False, _pool=None):
    """DevicePipeline.dc_correct_batch (see there)"""
    pool = pipe._pinned if _pool is None else _pool
    given = _batch_input(pipe, captures)
    iq, starts, d_mean = _dc_correct(pipe, pool, given)
    if want_means:
        return iq, starts, d_mean.cpu().numpy().reshape(len(given.lengths), 2)
    return iq, starts
