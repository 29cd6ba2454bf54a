"""What every batch call stages: the plan, the pinned staging buffers, THE upload in one copy, the noise blocks exchanged with the kernels."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib

_META_ALIGN = 256


def batch_step() -> int:
    """samples a wavefront of the batch kernel takes per step"""
    return int(_lib.load().urhgpu_batch_step())


def batch_plan(lengths, cp, cap_rows=None):
    """urhgpu_batch_plan: (plan int64[3 K] = region offsets, row capacities, launch order; work bytes; blob capacity).
    cap_rows: None = policy 0 (the stream's formula with a floor of 64 rows), "bound" = policy 1 (n / (tolerance + 1) + 2: cannot
    truncate), an int = that capacity for every capture.  Host arithmetic: works without a GPU."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    k = int(lengths.size)
    if cap_rows is None:
        policy, fixed = 0, 0
    elif isinstance(cap_rows, str):
        if cap_rows != "bound":
            raise ValueError('cap_rows is None, "bound" or an int')
        policy, fixed = 1, 0
    else:
        policy, fixed = 2, int(cap_rows)
    plan = np.zeros(3 * k, np.int64)
    work, blob = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().urhgpu_batch_plan(lengths.ctypes.data_as(C.c_void_p), k, C.byref(cp), policy, fixed, plan.ctypes.data_as(C.c_void_p),
                                             C.byref(work), C.byref(blob)))
    return plan, int(work.value), int(blob.value)


def order_params(modulation="FSK"):
    """parameters of a call that reads of them the plan's launch order and the sample type alone, or the modulation beside those (the estimate)"""
    from ..pipeline import DemodParams
    return DemodParams(modulation, 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)


def _pinned(torch, pool, key, nbytes):
    buf = pool.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes) + int(nbytes) // 4, 4096), dtype=torch.uint8).pin_memory()
        pool[key] = buf
    return buf


def _idle_stage(torch, pool, key, nbytes):
    """a pinned staging buffer of a call that RETURNS WITHOUT WAITING for its upload: the pool keeps, under `key`, the buffers handed out so
    far with the event recorded behind each one's copy (_stage_in_flight), and a buffer is handed out again only when that event has completed
    -- the next call must not rewrite bytes a queued copy has yet to read.  None is idle (or large enough): a new one."""
    ring = pool.setdefault(key, [])
    for item in list(ring):
        event, buf = item
        if event.query():
            ring.remove(item)
            if buf.numel() >= nbytes:
                return buf
    return torch.empty(max(int(nbytes) + int(nbytes) // 4, 4096), dtype=torch.uint8).pin_memory()


def _stage_in_flight(torch, pool, key, buf, stream):
    event = torch.cuda.Event()
    event.record(stream)
    pool[key].append((event, buf))


def captures_at(caps, starts, item):
    """a payload filler: every host capture's bytes at its start, `item` bytes per sample"""
    def fill(payload):
        for a, s in zip(caps, starts[:-1]):
            if len(a):
                payload[int(s) * item:(int(s) + len(a)) * item] = a.reshape(-1).view(np.uint8)
    return fill


# what upload() staged and queued: the device buffer and the addresses inside it, the staging buffer and the stream its copy runs on
Upload = namedtuple("Upload", "dev_in stage stream meta_bytes in_bytes d_start d_plan d_tables d_payload")


def upload(pipe, stage_for, device_for, starts, plan, tables=(), payload_bytes=0, fill=None) -> Upload:
    """THE upload of a batch call: int64 starts[K + 1], plan[3 K] and further int64 tables (the record map, the segmentation's regions) back to
    back, rounded up to _META_ALIGN bytes, then the payload (samples as bytes, float32 thresholds, noise blocks; fill(payload) writes it) --
    staged in pinned memory and queued as ONE copy on torch's current stream, which the context is set to first.  Which buffers is the caller's
    business: stage_for(bytes) hands out the pinned staging buffer (a key of the pool, or the idle ring of a call that does not wait),
    device_for(bytes) the device buffer (pooled under a key, or a tensor of this call alone), both at least that long."""
    torch = pipe.torch
    k = len(starts) - 1
    n_meta = 4 * k + 1 + sum(len(t) for t in tables)
    meta_bytes = (8 * n_meta + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
    in_bytes = meta_bytes + int(payload_bytes)
    stage = stage_for(in_bytes)
    view = stage.numpy()
    meta = view[:8 * n_meta].view(np.int64)
    meta[:k + 1] = starts
    meta[k + 1:4 * k + 1] = plan
    at = 4 * k + 1
    for t in tables:
        meta[at:at + len(t)] = t
        at += len(t)
    if fill is not None:
        fill(view[meta_bytes:in_bytes])
    stream = torch.cuda.current_stream(pipe.device)
    pipe.ctx.set_stream(stream.cuda_stream)
    dev_in = device_for(in_bytes)
    dev_in[:in_bytes].copy_(stage[:in_bytes], non_blocking=True)
    d_start = dev_in.data_ptr()
    return Upload(dev_in, stage, stream, meta_bytes, in_bytes, d_start, d_start + 8 * (k + 1), d_start + 8 * (4 * k + 1), d_start + meta_bytes)


def noise_buffer(pipe, k):
    """the device memory of K urhgpu_noise_result blocks"""
    return pipe._buf("batch:noise", (C.sizeof(_lib.NoiseResult) * max(k, 1),), pipe.torch.uint8)


def detect_noise(pipe, pool, d_iq, total, d_start, d_plan, k, cp):
    """AutoInterpretation.detect_noise_level of every capture alone: k_batch_noise and one read of the K blocks -> (values, flags)"""
    d_noise = noise_buffer(pipe, k)
    _lib.check(_lib.load().urhgpu_batch_noise_dev(pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), C.c_void_p(d_plan), k, C.byref(cp),
                                                  C.c_void_p(d_noise.data_ptr())))
    return read_noise_blocks(pipe, pool, d_noise, k)


def read_noise_blocks(pipe, pool, d_noise, k):
    """urhgpu_batch_noise_fetch: one read of the K result blocks -> (values as Python floats, flags)"""
    h = _pinned(pipe.torch, pool, "batch_noise", C.sizeof(_lib.NoiseResult) * max(k, 1))
    _lib.check(_lib.load().urhgpu_batch_noise_fetch(pipe.ctx.handle, C.c_void_p(d_noise.data_ptr()), k, C.c_void_p(h.data_ptr())))
    blocks = (_lib.NoiseResult * k).from_address(h.data_ptr())
    return [float(r.noise) for r in blocks], [int(r.flag) for r in blocks]


def write_noise_blocks(address, noise):
    """a result block per threshold at `address` (zeroed) as k_batch_noise leaves it for flag 1: the value, its float32, that one's fp32 square"""
    blocks = (_lib.NoiseResult * len(noise)).from_address(address)
    for r, value in zip(blocks, noise):
        f = np.float32(value)
        r.noise, r.noise_f32, r.noise_sqrd, r.flag = float(value), float(f), float(f * f), 1


def launch_counts(pipe):
    """(kernel launches, copies) the batch entry points have issued on the pipeline's context so far: 3 and 2 per batch, 4 and 3 per batch
    with automatic noise thresholds, 1 and 1 per detect_noise_levels; iq_to_bits_batch_center: 4 + 14 ceil(K / group) launches (5 + ... with
    automatic noise) and 3 copies (4), plus -- whatever the number of tied captures -- 3 launches and 3 copies when any center was left to the host;
    iq_to_bits_batch_records adds 3 launches and 1 copy to its batch, and as many to the second slicing of the captures left to the host;
    iq_to_bits_batch_psk: 4 launches (5 with automatic noise) and the copies of the matching batch above, with a center per capture
    14 ceil(K / group) launches more and the center's copies; costas_demod_batch: 1 launch; dc_correct_batch: 2 launches, and
    iq_to_bits_batch_dc those 2 more than its batch"""
    out = (C.c_int64 * 2)()
    _lib.check(_lib.load().urhgpu_batch_launches(pipe.ctx.handle, out))
    return int(out[0]), int(out[1])
