"""The walk's buffers, the fetch of the result blobs and the HostBits made of them, the messages' records behind a walk, and the walk alone."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib
from ..host_bits import HostBits
from .options import as_fsk
from .staging import _pinned, batch_plan, upload

# the pinned host buffer the blobs are first fetched into; a batch whose blobs are larger is told so by the fetch (which has read the
# directory by then), grows the buffer to what the directory says and fetches once more
FIRST_BLOB_BUFFER_BYTES = 8 << 20


# the device memory of a walk: the work regions, the counts, the directory and the blobs, with the two planned sizes
WalkBuffers = namedtuple("WalkBuffers", "work work_bytes counts d_dir blob blob_cap")


def walk_buffers(pipe, k, work_bytes, blob_cap) -> WalkBuffers:
    torch = pipe.torch
    return WalkBuffers(pipe._buf("batch:work", (max(work_bytes, 16),), torch.uint8), work_bytes, pipe._buf("batch:counts", (8 * max(k, 1),), torch.int64),
                       pipe._buf("batch:dir", (k + 1,), torch.int64), pipe._buf("batch:blob", (max(blob_cap, 16),), torch.uint8), blob_cap)


def _fetch_blobs(pipe, pool, d_dir, k, blob, blob_cap, tag=""):
    """urhgpu_batch_fetch into pinned memory of the pool: (directory, blobs)"""
    torch, lib = pipe.torch, _lib.load()
    h_dir = _pinned(torch, pool, "batch_dir" + tag, 8 * (k + 1))
    h_blob = _pinned(torch, pool, "batch_blob" + tag, min(blob_cap, FIRST_BLOB_BUFFER_BYTES))
    got = C.c_int64(0)

    def fetch():
        return lib.urhgpu_batch_fetch(pipe.ctx.handle, C.c_void_p(d_dir.data_ptr()), k, C.c_void_p(blob.data_ptr()), C.c_void_p(h_dir.data_ptr()),
                                      C.c_void_p(h_blob.data_ptr()), int(h_blob.numel()), C.byref(got))
    st = fetch()
    if st == _lib.ERR_CAPACITY and int(got.value) > h_blob.numel():
        h_blob = _pinned(torch, pool, "batch_blob" + tag, int(got.value))          # larger than the buffer so far: grow to what it needs, fetch again
        st = fetch()
    _lib.check(st)
    if int(got.value) > blob_cap:
        raise _lib.UrhGpuError(_lib.ERR_CAPACITY, "the batch's blobs did not fit the planned capacity")
    return h_dir, h_blob


def items_from_blobs(fetched, k, p, n_samples, qad, starts):
    """a HostBits per capture at the directory's offsets in what _fetch_blobs fetched; capture j's demodulated signal lies at qad[starts[j]]"""
    h_dir, h_blob = fetched
    offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
    items = []
    for j in range(k):
        h = HostBits.from_blob(h_blob.data_ptr() + int(offs[j]), p, seq=j, n_samples=int(n_samples[j]),
                               d_qad=(qad.data_ptr() + 4 * int(starts[j])) if qad is not None else 0)
        h._keep = (h_blob, qad)
        items.append(h)
    return items


# where the samples the records read lie: the buffer, its samples, the starts of its k_all captures, the parameters with the sample type
RecordSource = namedtuple("RecordSource", "d_iq total d_start k_all cp")


def record_capacity(plan):
    """records a batch with this plan can need at most: a region holds cap_rows / 2 + 1 messages (host arithmetic)"""
    k = len(plan) // 3
    return int((np.asarray(plan[k:2 * k], dtype=np.int64) // 2 + 1).sum())


def _queue_records(pipe, src, d_map, d_plan, k, plan, divisor, d_noise, bufs, tag=""):
    """urhgpu_batch_msg_records_dev behind the batch pass that has just filled the walk's work buffer and counts (bufs): three launches,
    nothing waited for.  d_map: None, or the device address of int64[K], the capture of src each of these K was demodulated from.
    Returns (device records, capacity)."""
    torch = pipe.torch
    cap_rec = record_capacity(plan)
    d_rec = pipe._buf("batch:rec" + tag, (C.sizeof(_lib.MsgRecord) * max(cap_rec, 1),), torch.uint8)
    d_cap = pipe._buf("batch:rec_capture" + tag, (max(cap_rec, 1),), torch.int32)
    d_dir = pipe._buf("batch:rec_dir" + tag, (k + 1,), torch.int64)
    _lib.check(_lib.load().urhgpu_batch_msg_records_dev(
        pipe.ctx.handle, C.c_void_p(src.d_iq), src.total, C.c_void_p(src.d_start), src.k_all, C.c_void_p(d_map) if d_map else None, C.c_void_p(d_plan), k,
        C.byref(src.cp), C.c_void_p(d_noise.data_ptr()) if d_noise is not None else None, int(divisor), C.c_void_p(bufs.work.data_ptr()), bufs.work_bytes,
        C.c_void_p(bufs.counts.data_ptr()), C.c_void_p(d_dir.data_ptr()), C.c_void_p(d_rec.data_ptr()), cap_rec, C.c_void_p(d_cap.data_ptr())))
    return d_rec, cap_rec


def _fetch_records(pipe, pool, queued, items, tag=""):
    """urhgpu_batch_records_fetch: ONE copy of the 32 M bytes in use -- M is the sum of the blob headers' n_msg, the records lie compacted in
    the captures' order -- and every HostBits gets its slice as .records (a view of pinned memory, valid as long as the blobs)"""
    from ..protocol import RECORD_DTYPE
    d_rec, cap_rec = queued
    n_msg = [int(h.n_msg) for h in items]
    total = sum(n_msg)
    h_rec = _pinned(pipe.torch, pool, "batch_rec" + tag, RECORD_DTYPE.itemsize * max(total, 1))
    _lib.check(_lib.load().urhgpu_batch_records_fetch(pipe.ctx.handle, C.c_void_p(d_rec.data_ptr()), total, cap_rec, C.c_void_p(h_rec.data_ptr())))
    rec = h_rec.numpy()[:RECORD_DTYPE.itemsize * total].view(RECORD_DTYPE)
    at = 0
    for h, n in zip(items, n_msg):
        h.records = rec[at:at + n]
        h._keep = (h._keep, h_rec)
        at += n


def _walk_qad(pipe, pool, qad, starts, p, thresholds, cap_rows, tag="", records=None):
    """urhgpu_qad_to_bits_batch_dev and its fetch on the captures qad[starts[j]:starts[j + 1]] (a device float32 tensor): the walk, scan and
    pack -- three launches --, one upload (starts, plan and the thresholds), two copies back.  thresholds: None (p.center for all) or
    float32 [K][order - 1].  records: None, or (message_length_divisor, where the samples lie -- RecordSource --, int64[K]: the capture
    of that buffer each of these was demodulated from): the records of this slicing are queued behind the walk and fetched, the map
    uploaded with the starts -- three more launches and one more copy.  Returns the HostBits list; their views live in pinned memory named
    by `tag`."""
    torch = pipe.torch
    starts = np.asarray(starts, dtype=np.int64)
    k = len(starts) - 1
    lengths = np.diff(starts)
    cp = as_fsk(p).to_c(np.float32)            # (PSK reaches this walk from iq_to_bits_batch_psk's second slicing alone: its FSK form serves)
    cp.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch_plan(lengths, cp, cap_rows)
    n_thr = 0 if thresholds is None else int(thresholds.size)

    def fill(payload):
        if n_thr:
            payload.view(np.float32)[:] = thresholds.reshape(-1)
    # THE upload: starts, plan, with records the map, and the thresholds in one copy
    up = upload(pipe, lambda n: _pinned(torch, pool, "batch_stage" + tag, n), lambda n: pipe._buf("batch:walk_in" + tag, (n,), torch.uint8), starts, plan,
                tables=() if records is None else (records[2],), payload_bytes=4 * n_thr, fill=fill)
    bufs = walk_buffers(pipe, k, work_bytes, blob_cap)
    _lib.check(_lib.load().urhgpu_qad_to_bits_batch_dev(pipe.ctx.handle, C.c_void_p(qad.data_ptr()), int(qad.shape[0]), C.c_void_p(up.d_start),
                                                        C.c_void_p(up.d_plan), k, C.byref(cp), C.c_void_p(up.d_payload) if n_thr else None, n_thr, None,
                                                        C.c_void_p(bufs.work.data_ptr()), work_bytes, C.c_void_p(bufs.counts.data_ptr()),
                                                        C.c_void_p(bufs.d_dir.data_ptr()), C.c_void_p(bufs.blob.data_ptr()), blob_cap))
    queued = None
    if records is not None:
        queued = _queue_records(pipe, records[1], up.d_tables, up.d_plan, k, plan, records[0], None, bufs, tag)
    items = items_from_blobs(_fetch_blobs(pipe, pool, bufs.d_dir, k, bufs.blob, bufs.blob_cap, tag), k, p, lengths, qad, starts)
    if queued is not None:
        _fetch_records(pipe, pool, queued, items, tag)
    return items
