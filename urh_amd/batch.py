"""Many short captures in one pass (include/urhgpu.h "a batch of captures"; urh_amd/csrc/batch.hip).

A pass over one capture is all fixed cost below a few hundred thousand samples; a recording session is a directory of hundreds or
thousands of such captures.  DevicePipeline.iq_to_bits_batch packs them into ONE pinned staging buffer, uploads it with one copy, has
three launches demodulate and digitise all of them (a wavefront per capture), and fetches every capture's compact result blob with one
copy.  The results are HostBits made at the directory's offsets: no new result format.  Long captures still belong to passes and
streams -- a wavefront walks its capture serially --, so a capture of `long_from` samples or more is routed through the ordinary
iq_to_bits and takes its place in the sequence.

DevicePipeline.iq_to_bits_batch_auto opens the captures the way the reference opens each of its files: one more launch in front
(k_batch_noise, urh_amd/csrc/batch_auto.hip) runs AutoInterpretation.detect_noise_level on every capture, and the walk gates each capture
with its own threshold -- four launches and three read-backs whatever the number of captures.  detect_noise_levels is that first launch
alone.

DevicePipeline.iq_to_bits_batch_center also slices every capture with its OWN center (urh_amd/csrc/batch_center.hip): the captures are
demodulated into one buffer, one chain of kernels runs AutoInterpretation.detect_center on all of them, and the walk classifies each
capture through the thresholds of its center.  Where the device leaves a center to numpy (more bins than its pool holds, a tie between
the second and the third peak) the host settles it and ALL those captures are sliced again by one more call.  detect_centers is the chain
alone, qad_to_bits_batch the walk alone.

DevicePipeline.iq_to_bits_batch_records ends any of the three with the session's MESSAGES: one record per message (RSSI, first position,
ASK padding) queued behind the walk for all captures at once (urh_amd/csrc/batch_records.hip) -- three more launches and one more copy,
whatever the number of captures and of messages.  BatchBits.messages() is then what ProtocolAnalyzer.get_protocol_from_signal builds per file.

DevicePipeline.estimate_batch stands in front of all of them: AutoInterpretation.estimate of every capture -- modulation, samples per symbol,
center, tolerance, noise --, with the captures' message ranges from three launches (urh_amd/csrc/batch_estimate.hip: a wavefront per capture
follows segment_messages_from_magnitudes) and the messages of all captures pooled through the native calls estimators.estimate_dev makes for one
capture.  segment_messages_batch is the segmentation alone.

DevicePipeline.iq_to_bits_batch_psk is the batch of PSK captures (urh_amd/csrc/batch_psk.hip): ONE launch runs the Costas loop of every
capture -- a lane per capture, each from the known start state, nothing speculated -- into the demodulated buffer, and the route of
iq_to_bits_batch_center goes on from there (the center chain only when asked for, the qad-input walk, the records) with the parameters
recoded as FSK, whose noise value PSK shares.  The loop is serial: the device time follows the LONGEST capture of the batch, not their
number.  costas_demod_batch is that launch alone.  The entry points above keep refusing PSK and name this one.

DevicePipeline.iq_to_bits_batch_dc is any of the above over captures minus their own means -- the reference's DC correction, the default of
its receive path (urh_amd/csrc/batch_dc.hip): TWO launches in front correct every capture on the device, bit-equal with numpy's expression
(for float32 captures numpy's strictly sequential column sum, a lane per capture and column), and the matching batch runs on the corrected
buffer.  dc_correct_batch is those two launches alone; what it returns is the third input form of every batch method.  The entry points
above keep refusing dc_correction and name this one.
"""
import ctypes as C
from dataclasses import replace

import numpy as np

from . import _lib
from .host_bits import HostBits
from .signal_functions import mod_code

# a capture of this many samples or more goes through an ordinary pass: the capture length at which a batch's wavefront per capture stops
# beating a pipelined stream's pass per capture -- measured: B / A = 1.39 at 131 072 samples, 1.02 and 0.98 at 196 608 (two runs), 0.98 at 262 144
# (tools/batch_probe.py, profiles/batch_probe.txt; DESIGN.md 7.7e has the table).  PSK keeps it: no measured set has the stream ahead of
# iq_to_bits_batch_psk at or below it -- B / A = 22.7 for 341 captures of 196 608 samples (tools/batch_psk_probe.py,
# profiles/batch_psk_probe.txt)
LONG_FROM_DEFAULT = 196_608

# the refusals of dc_correction name the entry point that does it, then say what they always said
_DC_FIRST = "call iq_to_bits_batch_dc(captures, p, ...), which removes every capture's means on the device in two more launches; apart from that method "

_NOT_IN_A_BATCH = {
    "auto_center": "iq_to_bits_batch slices every capture with p.center: call iq_to_bits_batch_center(captures, p, auto_noise=False), which detects a center "
                   "per capture (or call iq_to_bits(..., auto_center=True) per capture, or a CaptureStream(auto_center=True))",
    "auto_noise": "iq_to_bits_batch gates every capture with p.noise_threshold: call iq_to_bits_batch_auto(captures, p), which detects a threshold per capture",
    "msg_records": "iq_to_bits_batch computes no message records: call iq_to_bits_batch_records(captures, p), which queues them behind the batch (or call "
                   "iq_to_bits(..., msg_records=True) per capture, or a CaptureStream(msg_records=True))",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., dc_correction=True) per capture, or a CaptureStream(dc_correction=True)",
}


def check_batch_options(p, **options):
    """what a batch does not do raises ValueError with a sentence that says what to call instead (host arithmetic: no GPU needed)"""
    for name, value in options.items():
        if name not in _NOT_IN_A_BATCH:
            raise TypeError(f"iq_to_bits_batch() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {_NOT_IN_A_BATCH[name]}")
    mod, _ = mod_code(p.modulation_type)
    if mod not in (_lib.MOD_ASK, _lib.MOD_FSK):
        raise ValueError(f"this batch demodulates ASK and FSK, not {p.modulation_type}: for PSK call iq_to_bits_batch_psk(captures, p), which runs a "
                         "Costas loop per capture in one launch (or call iq_to_bits per capture, or push the captures through a CaptureStream)")


def is_psk(p) -> bool:
    return mod_code(p.modulation_type)[0] == _lib.MOD_PSK


def as_fsk(p):
    """PSK parameters recoded as FSK for what reads no modulation but through the noise value, which the two share (-4): the plan (lengths,
    tolerance, samples per symbol, bits per symbol), the qad-input walk (no ASK rule) and the records (no ASK padding)"""
    return replace(p, modulation_type="FSK") if is_psk(p) else p


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


def route(lengths, long_from=None):
    """(indices of the captures the batch takes, indices of those that go through an ordinary pass: long_from samples or more)"""
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.nonzero(lengths < long_from)[0], np.nonzero(lengths >= long_from)[0]


class BatchBits:
    """The results of a batch: a sequence of HostBits, one per capture in the order given (ppseq(), bits(), msg_off, pauses,
    bit_sample_pos(), pos_offsets(), flat(), truncated, rows_needed, check() as for a stream's results).  Views of pinned memory of the
    pipeline: valid until its next batch; copy what has to live longer."""

    def __init__(self, items, params, lengths, qads=None, rerun=None, noise=None, noise_flags=None, centers=None, center_flags=None, means=None):
        self._items = list(items)
        # iq_to_bits_batch_dc: the two means taken off every capture, numpy [K, 2] (float32 for float32 captures, float64 otherwise; NaN for
        # an empty capture)
        self.means = means
        self.params = params
        self.lengths = [int(n) for n in lengths]
        self._qads = qads                  # per capture: device tensor or None
        self._rerun = rerun                # k, cap_rows -> (HostBits, qad)
        # iq_to_bits_batch_auto: detect_noise_level's value per capture (Python floats) and urhgpu_noise_result's flag per capture -- 1 the
        # capture was gated with its value; 2 the value is not below the sample type's max_magnitude: the reference slices zeros(2), and so
        # did the batch (n_samples = 2); 0 the reference raises, and so does handing that capture out (the value is the NaN / infinity)
        self.noise = None if noise is None else [float(x) for x in noise]
        self.noise_flags = None if noise_flags is None else [int(f) for f in noise_flags]
        # iq_to_bits_batch_center: detect_center's value per capture (a Python float, or None where it gives None: the capture was sliced
        # with p.center) and urhgpu_center_result's flag per capture AS THE DEVICE REPORTED IT -- 1 decided on the device, 0 None, 2 / 3
        # left to the host: settled before the method returned, the capture sliced again with the settled center
        self.centers = None if centers is None else [None if c is None else float(c) for c in centers]
        self.center_flags = None if center_flags is None else [int(f) for f in center_flags]

    def __len__(self):
        return len(self._items)

    def _hand_out(self, k):
        if self.noise_flags is not None and self.noise_flags[k] == 0:
            from .pipeline import raise_noise_error
            raise_noise_error(self.noise[k])               # what detect_noise_level raises for this capture; the others are handed out
        return self._items[k]

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self._hand_out(i) for i in range(*k.indices(len(self._items)))]      # (a slice gives a list of HostBits)
        return self._hand_out(range(len(self._items))[k])

    def __iter__(self):
        return (self._hand_out(k) for k in range(len(self._items)))

    @property
    def truncated(self):
        """indices of the captures whose results did not fit their capacities"""
        return [k for k, h in enumerate(self._items) if h is not None and h.truncated]

    def check(self):
        for k in range(len(self._items)):
            self._hand_out(k).check()
        return self

    def qad(self, k):
        """capture k's demodulated signal: its slice of the batch's device tensor (want_qad=True)"""
        if self._qads is None:
            raise ValueError("the batch did not keep the demodulated signal (want_qad=True)")
        return self._qads[k]

    def message_data(self, k, sample_rate=1e6, timestamp=0.0):
        """iq_to_bits_batch_records: capture k's list of protocol.MessageData (HostBits.message_data); a truncated capture raises the
        capacity error -- retry(k) runs it again, records included"""
        return self[k].message_data(sample_rate, timestamp)

    def messages(self, sample_rate=1e6, timestamps=None):
        """iq_to_bits_batch_records: the session's messages, a list of MessageData per capture in the order given.  timestamps: one per
        capture (Signal.timestamp of that file), default 0.0 for all"""
        if timestamps is not None and len(timestamps) != len(self._items):
            raise ValueError("timestamps holds one entry per capture")
        return [self.message_data(k, sample_rate, 0.0 if timestamps is None else timestamps[k]) for k in range(len(self._items))]

    def retry(self, k):
        """a truncated capture once more, alone, with the row capacity its first run reported; the result (with its records, where the
        batch computed them) takes its place"""
        if self._rerun is None:
            raise ValueError("this result cannot run a capture again")
        h = self._items[k]
        again, qad = self._rerun(k, max(int(h.rows_needed), 1))
        self._items[k] = again
        if self._qads is not None:
            self._qads[k] = qad
        return again


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


def _pinned(torch, pool, key, nbytes):
    buf = pool.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes) + int(nbytes) // 4, 4096), dtype=torch.uint8).pin_memory()
        pool[key] = buf
    return buf


_META_ALIGN = 256

# the pinned host buffer the blobs are first fetched into; a batch whose blobs are larger is told so by the fetch (which has read the
# directory by then), grows the buffer to what the directory says and fetches once more
FIRST_BLOB_BUFFER_BYTES = 8 << 20


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


def _center_buffers(pipe, k, total, order, cap_tie, max_bins=None):
    """the device memory of the chain's scratch and outputs: (scratch, bytes, thr, cap_thr, res, tie, cap_tie)"""
    torch = pipe.torch
    max_bins = int(_lib.load().urhgpu_center_hist_cap(pipe.ctx.handle)) if max_bins is None else max_bins
    scratch_bytes, _, _ = batch_center_plan(np.zeros(k, np.int64), total, max_bins)
    cap_tie = TIE_POOL_COUNTS_PER_CAPTURE * max(k, 1) if cap_tie is None else int(cap_tie)
    scratch = pipe._buf("batch:center_scratch", (max(scratch_bytes, 256),), torch.uint8)
    cap_thr = max(k * (order - 1), 1)
    thr = pipe._buf("batch:thr", (cap_thr,), torch.float32)
    res = pipe._buf("batch:center_res", (C.sizeof(_lib.BatchCenterResult) * (k + 1),), torch.uint8)
    tie = pipe._buf("batch:tie", (max(cap_tie, 1),), torch.int32)
    return scratch, scratch_bytes, thr, cap_thr, res, tie, cap_tie


def _fetch_centers(pipe, pool, res, k, tie, cap_tie):
    """urhgpu_batch_center_fetch: (the K result blocks, the used part of the tie pool as uint32) -- two copies at most"""
    torch, lib = pipe.torch, _lib.load()
    h_res = _pinned(torch, pool, "batch_center_res", C.sizeof(_lib.BatchCenterResult) * (k + 1))
    h_tie = _pinned(torch, pool, "batch_tie", 4 * max(cap_tie, 1))
    used = C.c_int64(0)
    _lib.check(lib.urhgpu_batch_center_fetch(pipe.ctx.handle, C.c_void_p(res.data_ptr()), k, C.c_void_p(tie.data_ptr()), cap_tie, C.c_void_p(h_res.data_ptr()),
                                             C.c_void_p(h_tie.data_ptr()), cap_tie, C.byref(used)))
    blocks = (_lib.BatchCenterResult * (k + 1)).from_address(h_res.data_ptr())
    return blocks, h_tie.numpy()[:4 * int(used.value)].view(np.uint32)


def _settle_centers(pipe, blocks, counts, k, qad, starts, n_of, max_size, skip=()):
    """(centers, flags as the device reported them, indices whose center the HOST settled to a value) for the K result blocks: flag 1 -- the
    device's center; 0 -- None; 3 with the histogram in the tie pool -- pipeline.decide_center on the shipped counts; 2, and a tie that did
    not fit the pool -- the single-range estimator on the capture's slice of qad.  skip: captures that are not handed out (noise flag 0)."""
    from .pipeline import decide_center
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


def record_capacity(plan):
    """records a batch with this plan can need at most: a region holds cap_rows / 2 + 1 messages (host arithmetic)"""
    k = len(plan) // 3
    return int((np.asarray(plan[k:2 * k], dtype=np.int64) // 2 + 1).sum())


def _queue_records(pipe, src, d_map, d_plan, k, plan, divisor, d_noise, work, work_bytes, counts, tag=""):
    """urhgpu_batch_msg_records_dev behind the batch pass that has just filled work and counts: three launches, nothing waited for.
    src: where the samples lie -- (d_iq, total, d_start, k_all, the parameters with the sample type).  Returns (device records, capacity)."""
    torch = pipe.torch
    d_iq, total, d_start, k_all, cp = src
    cap_rec = record_capacity(plan)
    d_rec = pipe._buf("batch:rec" + tag, (C.sizeof(_lib.MsgRecord) * max(cap_rec, 1),), torch.uint8)
    d_cap = pipe._buf("batch:rec_capture" + tag, (max(cap_rec, 1),), torch.int32)
    d_dir = pipe._buf("batch:rec_dir" + tag, (k + 1,), torch.int64)
    _lib.check(_lib.load().urhgpu_batch_msg_records_dev(
        pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), k_all, C.c_void_p(d_map) if d_map else None, C.c_void_p(d_plan), k, C.byref(cp),
        C.c_void_p(d_noise.data_ptr()) if d_noise is not None else None, int(divisor), C.c_void_p(work.data_ptr()), work_bytes, C.c_void_p(counts.data_ptr()),
        C.c_void_p(d_dir.data_ptr()), C.c_void_p(d_rec.data_ptr()), cap_rec, C.c_void_p(d_cap.data_ptr())))
    return d_rec, cap_rec


def _fetch_records(pipe, pool, queued, items, tag=""):
    """urhgpu_batch_records_fetch: ONE copy of the 32 M bytes in use -- M is the sum of the blob headers' n_msg, the records lie compacted in
    the captures' order -- and every HostBits gets its slice as .records (a view of pinned memory, valid as long as the blobs)"""
    from .protocol import RECORD_DTYPE
    torch = pipe.torch
    d_rec, cap_rec = queued
    n_msg = [int(h.n_msg) for h in items]
    total = sum(n_msg)
    h_rec = _pinned(torch, pool, "batch_rec" + tag, RECORD_DTYPE.itemsize * max(total, 1))
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
    float32 [K][order - 1].  records: None, or (message_length_divisor, where the samples lie -- _queue_records' src --, int64[K]: the capture
    of that buffer each of these was demodulated from): the records of this slicing are queued behind the walk and fetched, the map
    uploaded with the starts -- three more launches and one more copy.  Returns the HostBits list; their views live in pinned memory named
    by `tag`."""
    torch, lib = pipe.torch, _lib.load()
    starts = np.asarray(starts, dtype=np.int64)
    k = len(starts) - 1
    lengths = np.diff(starts)
    cp = as_fsk(p).to_c(np.float32)            # (PSK reaches this walk from iq_to_bits_batch_psk's second slicing alone: its FSK form serves)
    cp.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch_plan(lengths, cp, cap_rows)
    n_thr = 0 if thresholds is None else int(thresholds.size)
    n_meta = 4 * k + 1 + (k if records is not None else 0)                     # starts, plan and -- with records -- the map
    meta_bytes = (8 * n_meta + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
    stage = _pinned(torch, pool, "batch_stage" + tag, meta_bytes + 4 * n_thr)
    view = stage.numpy()
    meta = view[:8 * n_meta].view(np.int64)
    meta[:k + 1] = starts
    meta[k + 1:4 * k + 1] = plan
    if records is not None:
        meta[4 * k + 1:] = records[2]
    if n_thr:
        view[meta_bytes:meta_bytes + 4 * n_thr].view(np.float32)[:] = thresholds.reshape(-1)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    dev_in = pipe._buf("batch:walk_in" + tag, (meta_bytes + 4 * n_thr,), torch.uint8)
    dev_in.copy_(stage[:meta_bytes + 4 * n_thr], non_blocking=True)                  # THE upload: starts, plan and thresholds in one copy
    work = pipe._buf("batch:work", (max(work_bytes, 16),), torch.uint8)
    counts = pipe._buf("batch:counts", (8 * max(k, 1),), torch.int64)
    d_dir = pipe._buf("batch:dir", (k + 1,), torch.int64)
    blob = pipe._buf("batch:blob", (max(blob_cap, 16),), torch.uint8)
    _lib.check(lib.urhgpu_qad_to_bits_batch_dev(pipe.ctx.handle, C.c_void_p(qad.data_ptr()), int(qad.shape[0]), C.c_void_p(dev_in.data_ptr()),
                                                C.c_void_p(dev_in.data_ptr() + 8 * (k + 1)), k, C.byref(cp),
                                                C.c_void_p(dev_in.data_ptr() + meta_bytes) if n_thr else None, n_thr, None, C.c_void_p(work.data_ptr()),
                                                work_bytes, C.c_void_p(counts.data_ptr()), C.c_void_p(d_dir.data_ptr()), C.c_void_p(blob.data_ptr()), blob_cap))
    queued = None
    if records is not None:
        queued = _queue_records(pipe, records[1], dev_in.data_ptr() + 8 * (4 * k + 1), dev_in.data_ptr() + 8 * (k + 1), k, plan, records[0], None, work,
                                work_bytes, counts, tag)
    h_dir, h_blob = _fetch_blobs(pipe, pool, d_dir, k, blob, blob_cap, tag)
    offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
    items = []
    for j in range(k):
        h = HostBits.from_blob(h_blob.data_ptr() + int(offs[j]), p, seq=j, n_samples=int(lengths[j]), d_qad=qad.data_ptr() + 4 * int(starts[j]))
        h._keep = (h_blob, qad)
        items.append(h)
    if queued is not None:
        _fetch_records(pipe, pool, queued, items, tag)
    return items


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


def _run_batch(pipe, caps, lengths, npdt, p, want_qad, cap_rows, pool, device_iq=None, device_starts=None, auto_noise=False, center=None, records=None,
               psk=False):
    """the short captures of a batch through the three launches.  caps: numpy arrays (packed and uploaded here, one copy), or device_iq (a
    device tensor that holds them back to back) with device_starts.  auto_noise: four launches -- every capture gated with the threshold
    detected for it (urhgpu_iq_to_bits_batch_auto_dev) -- and one more read, of the K result blocks; "only": that first launch and that
    read alone.  center: None, or {"max_size", "cap_tie"} -- every capture sliced with its own center (urhgpu_iq_to_bits_batch_center_dev),
    the centers the device left to the host settled and those captures sliced again by ONE more call.  records: None, or the
    message_length_divisor -- the records of all captures are queued behind the walk (urhgpu_batch_msg_records_dev: before anything reuses
    the work buffer) and fetched with one copy; the captures sliced again get the records of their second slicing the same way.
    psk: the captures are demodulated by a Costas loop per capture (urhgpu_iq_to_bits_batch_psk_dev: one launch, into the qad buffer) and walked
    from there, with or without a center per capture; the plan, the walk and the records take the parameters recoded as FSK (as_fsk).
    Returns (HostBits list, qad tensor or None, device input, starts, (noise values, flags) or None, (centers, flags) or None)."""
    torch, lib = pipe.torch, _lib.load()
    k = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    cp = p.to_c(npdt)
    cp.write_bit_sample_pos = 0
    cp_walk = cp
    if psk:
        cp_walk = as_fsk(p).to_c(npdt)
        cp_walk.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch_plan(lengths, cp_walk, cap_rows)
    starts = np.zeros(k + 1, np.int64)
    np.cumsum(lengths, out=starts[1:])
    if device_starts is not None:
        starts = np.asarray(device_starts, dtype=np.int64)
    total = int(starts[-1]) if device_iq is None else int(device_iq.shape[0])
    item = 2 * np.dtype(npdt).itemsize
    meta_bytes = (8 * (4 * k + 1) + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
    in_bytes = meta_bytes + (total * item if device_iq is None else 0)
    stage = _pinned(torch, pool, "batch_stage", in_bytes)
    view = stage.numpy()
    meta = view[:8 * (4 * k + 1)].view(np.int64)
    meta[:k + 1] = starts
    meta[k + 1:] = plan
    if device_iq is None:
        for a, s in zip(caps, starts[:-1]):
            if len(a):
                view[meta_bytes + int(s) * item: meta_bytes + (int(s) + len(a)) * item] = a.reshape(-1).view(np.uint8)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    dev_in = torch.empty(in_bytes, dtype=torch.uint8, device=pipe.device)       # the result holds it: retry() reads its capture there
    dev_in.copy_(stage[:in_bytes], non_blocking=True)                            # THE upload: starts, plan and every sample in one copy
    d_start = dev_in.data_ptr()
    d_plan = d_start + 8 * (k + 1)
    d_iq = dev_in.data_ptr() + meta_bytes if device_iq is None else device_iq.data_ptr()
    d_noise = pipe._buf("batch:noise", (C.sizeof(_lib.NoiseResult) * max(k, 1),), torch.uint8) if auto_noise else None

    def fetch_noise():
        h = _pinned(torch, pool, "batch_noise", C.sizeof(_lib.NoiseResult) * max(k, 1))
        _lib.check(lib.urhgpu_batch_noise_fetch(pipe.ctx.handle, C.c_void_p(d_noise.data_ptr()), k, C.c_void_p(h.data_ptr())))
        blocks = (_lib.NoiseResult * k).from_address(h.data_ptr())
        return [float(r.noise) for r in blocks], [int(r.flag) for r in blocks]
    if auto_noise == "only":
        _lib.check(lib.urhgpu_batch_noise_dev(pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), C.c_void_p(d_plan), k, C.byref(cp_walk),
                                              C.c_void_p(d_noise.data_ptr())))
        return None, None, (dev_in, meta_bytes, device_iq), starts, fetch_noise(), None
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device) if (want_qad or center is not None or psk) else None
    work = pipe._buf("batch:work", (max(work_bytes, 16),), torch.uint8)
    counts = pipe._buf("batch:counts", (8 * max(k, 1),), torch.int64)
    d_dir = pipe._buf("batch:dir", (k + 1,), torch.int64)
    blob = pipe._buf("batch:blob", (max(blob_cap, 16),), torch.uint8)
    args = (pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), C.c_void_p(d_plan), k, C.byref(cp),
            C.c_void_p(qad.data_ptr()) if qad is not None else None, C.c_void_p(work.data_ptr()), work_bytes,
            C.c_void_p(counts.data_ptr()), C.c_void_p(d_dir.data_ptr()), C.c_void_p(blob.data_ptr()), blob_cap)
    if center is not None:
        max_size = -1 if center["max_size"] is None else int(center["max_size"])
        scratch, scratch_bytes, thr, cap_thr, res, tie, cap_tie = _center_buffers(pipe, k, total, 1 << p.bits_per_symbol, center.get("cap_tie"))
        outputs = (C.c_void_p(d_noise.data_ptr()) if auto_noise else None, C.c_void_p(scratch.data_ptr()), scratch_bytes, C.c_void_p(thr.data_ptr()),
                   cap_thr, C.c_void_p(res.data_ptr()), k + 1, C.c_void_p(tie.data_ptr()), cap_tie)
        if psk:
            _lib.check(lib.urhgpu_iq_to_bits_batch_psk_dev(*args[:7], 1 if auto_noise else 0, 1, max_size, *args[7:], *outputs))
        else:
            _lib.check(lib.urhgpu_iq_to_bits_batch_center_dev(*args[:7], 1 if auto_noise else 0, max_size, *args[7:], *outputs))
    elif psk:
        _lib.check(lib.urhgpu_iq_to_bits_batch_psk_dev(*args[:7], 1 if auto_noise else 0, 0, -1, *args[7:], C.c_void_p(d_noise.data_ptr()) if auto_noise else None,
                                                       None, 0, None, 0, None, 0, None, 0))
    elif auto_noise:
        _lib.check(lib.urhgpu_iq_to_bits_batch_auto_dev(*args, C.c_void_p(d_noise.data_ptr())))
    else:
        _lib.check(lib.urhgpu_iq_to_bits_batch_dev(*args))
    rec_src = (d_iq, total, d_start, k, cp_walk)
    queued = None if records is None else _queue_records(pipe, rec_src, None, d_plan, k, plan, records, d_noise, work, work_bytes, counts)
    h_dir, h_blob = _fetch_blobs(pipe, pool, d_dir, k, blob, blob_cap)
    noise = fetch_noise() if auto_noise else None
    offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
    items = []
    for i in range(k):
        n_i = 2 if (noise is not None and noise[1][i] == 2) else int(lengths[i])      # flag 2: the reference slices zeros(2), and so did the device
        h = HostBits.from_blob(h_blob.data_ptr() + int(offs[i]), p, seq=i, n_samples=n_i,
                               d_qad=(qad.data_ptr() + 4 * int(starts[i])) if qad is not None else 0)
        h._keep = (h_blob, qad)
        items.append(h)
    if queued is not None:
        _fetch_records(pipe, pool, queued, items)
    found = None
    if center is not None:
        blocks, tie_counts = _fetch_centers(pipe, pool, res, k, tie, cap_tie)
        n_of = lambda i: items[i].n_samples                                          # noqa: E731
        skip = {i for i in range(k) if noise is not None and noise[1][i] == 0}      # (the reference raises for these: nothing is handed out)
        centers, flags, settled = _settle_centers(pipe, blocks, tie_counts, k, qad, starts, n_of, center["max_size"], skip)
        if settled:
            # ALL the captures the host has settled a center for, sliced again by ONE call: their demodulated signals gathered back to back
            # (one torch.cat), the thresholds of their centers uploaded with the starts and the plan
            parts = [qad[int(starts[i]):int(starts[i]) + n_of(i)] for i in settled]
            sub = torch.cat(parts) if len(parts) > 1 else parts[0]
            sub_starts = np.concatenate([[0], np.cumsum([n_of(i) for i in settled])]).astype(np.int64)
            again = _walk_qad(pipe, pool, sub.contiguous(), sub_starts, p, center_thresholds(p, [centers[i] for i in settled]), cap_rows, tag=":again",
                              records=None if records is None else (records, rec_src, np.asarray(settled, dtype=np.int64)))
            for i, h in zip(settled, again):
                h.seq = i
                items[i] = h
        found = (centers, flags)
    return items, qad, (dev_in, meta_bytes, device_iq), starts, noise, found


def iq_to_bits_batch(pipe, captures, p, want_qad=False, cap_rows=None, long_from=None, _pool=None, **options):
    """DevicePipeline.iq_to_bits_batch (see there)"""
    check_batch_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, False)


_NOT_IN_A_BATCH_AUTO = {
    "auto_center": "iq_to_bits_batch_auto slices every capture with p.center: call iq_to_bits_batch_center(captures, p), which detects a threshold and a "
                   "center per capture (or call iq_to_bits(..., auto_noise=True, auto_center=True) per capture, or a CaptureStream)",
    "msg_records": "iq_to_bits_batch_auto computes no message records: call iq_to_bits_batch_records(captures, p, auto_noise=True), which queues them behind "
                   "the batch (or call iq_to_bits(..., auto_noise=True, msg_records=True) per capture, or a CaptureStream)",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., auto_noise=True, dc_correction=True) per capture, or a CaptureStream",
}


def check_batch_auto_options(p, **options):
    """what iq_to_bits_batch_auto does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    for name, value in options.items():
        if name not in _NOT_IN_A_BATCH_AUTO:
            raise TypeError(f"iq_to_bits_batch_auto() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {_NOT_IN_A_BATCH_AUTO[name]}")
    check_batch_options(p)


def iq_to_bits_batch_auto(pipe, captures, p, auto_noise=True, want_qad=False, cap_rows=None, long_from=None, _pool=None, **options):
    """DevicePipeline.iq_to_bits_batch_auto (see there)"""
    check_batch_auto_options(p, **options)
    if not auto_noise:
        return iq_to_bits_batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, True)


def detect_noise_levels(pipe, captures):
    """AutoInterpretation.detect_noise_level of every capture of a batch (the three input forms of iq_to_bits_batch): ONE launch and one
    read of the K result blocks, whatever K and the lengths are -- the batch counterpart of estimators.detect_noise_level_dev.  Returns the
    list of thresholds (Python floats; a value that is not below the sample type's max_magnitude is returned as it is); where the reference
    raises for a capture (math.ceil of a NaN / an infinity), so does this."""
    from .pipeline import DemodParams, raise_noise_error
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)            # (the detection reads the samples and the sample type alone)
    noise, flags = _batch(pipe, captures, p, False, None, 2 ** 31, None, "only")
    for value, flag in zip(noise, flags):
        if flag == 0:
            raise_noise_error(value)
    return noise


_NOT_IN_A_BATCH_CENTER = {
    "msg_records": "iq_to_bits_batch_center computes no message records: call iq_to_bits_batch_records(captures, p, auto_noise=..., auto_center=True), which "
                   "queues them behind the batch (or call iq_to_bits(..., auto_center=True, msg_records=True) per capture, or a CaptureStream)",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., auto_center=True, dc_correction=True) per capture, or a CaptureStream",
}


def check_batch_center_options(p, **options):
    """what iq_to_bits_batch_center does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    for name, value in options.items():
        if name not in _NOT_IN_A_BATCH_CENTER:
            raise TypeError(f"iq_to_bits_batch_center() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {_NOT_IN_A_BATCH_CENTER[name]}")
    check_batch_options(p)


def iq_to_bits_batch_center(pipe, captures, p, auto_noise=True, center_max_size=None, want_qad=False, cap_rows=None, long_from=None, _pool=None,
                            _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_center (see there)"""
    check_batch_center_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, bool(auto_noise), center={"max_size": center_max_size, "cap_tie": _cap_tie})


_NOT_IN_A_BATCH_RECORDS = {
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., msg_records=True, dc_correction=True) per capture, or a CaptureStream",
}


def check_batch_records_options(p, message_length_divisor=1, **options):
    """what iq_to_bits_batch_records does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    for name, value in options.items():
        if name not in _NOT_IN_A_BATCH_RECORDS:
            raise TypeError(f"iq_to_bits_batch_records() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {_NOT_IN_A_BATCH_RECORDS[name]}")
    check_batch_options(p)
    if not 1 <= int(message_length_divisor) <= 1 << 30:
        raise ValueError("message_length_divisor must be at least 1 (and at most 2 ** 30)")


def iq_to_bits_batch_records(pipe, captures, p, message_length_divisor=1, auto_noise=False, auto_center=False, center_max_size=None, want_qad=False,
                             cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_records (see there)"""
    check_batch_records_options(p, message_length_divisor, **options)
    center = {"max_size": center_max_size, "cap_tie": _cap_tie} if auto_center else None
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, bool(auto_noise), center=center, records=int(message_length_divisor))


_NOT_IN_A_BATCH_PSK = {
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., dc_correction=True) per capture, or a CaptureStream(dc_correction=True)",
}


def check_batch_psk_options(p, message_length_divisor=None, **options):
    """what iq_to_bits_batch_psk does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    for name, value in options.items():
        if name not in _NOT_IN_A_BATCH_PSK:
            raise TypeError(f"iq_to_bits_batch_psk() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {_NOT_IN_A_BATCH_PSK[name]}")
    if not is_psk(p):
        raise ValueError(f"iq_to_bits_batch_psk demodulates PSK, not {p.modulation_type}: for ASK and FSK call iq_to_bits_batch or one of its siblings "
                         "(iq_to_bits_batch_auto, iq_to_bits_batch_center, iq_to_bits_batch_records)")
    if message_length_divisor is not None and not 1 <= int(message_length_divisor) <= 1 << 30:
        raise ValueError("message_length_divisor must be at least 1 (and at most 2 ** 30)")


def iq_to_bits_batch_psk(pipe, captures, p, auto_noise=False, auto_center=False, center_max_size=None, message_length_divisor=None, want_qad=False,
                         cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_psk (see there)"""
    check_batch_psk_options(p, message_length_divisor, **options)
    center = {"max_size": center_max_size, "cap_tie": _cap_tie} if auto_center else None
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, bool(auto_noise), center=center,
                  records=None if message_length_divisor is None else int(message_length_divisor), psk=True)


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


def costas_demod_batch(pipe, captures, p, noise=None, _pool=None):
    """DevicePipeline.costas_demod_batch (see there)"""
    check_batch_psk_options(p)
    torch, lib = pipe.torch, _lib.load()
    pool = pipe._pinned if _pool is None else _pool
    caps, on_device, packed, cat, starts_in, npdt, lengths = _batch_input(pipe, captures)
    k = len(lengths)
    if noise is not None and len(noise) != k:
        raise ValueError("noise holds one threshold per capture (or is None: p.noise_threshold for all)")
    cp = p.to_c(npdt)
    plan, _, _ = batch_plan(lengths, as_fsk(p).to_c(npdt))
    starts = starts_in if packed else np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if on_device:
        iq = cat if packed else (torch.cat(caps) if caps else torch.empty((0, 2), dtype=torch.float32, device=pipe.device))
        iq = iq.contiguous()
        total = int(iq.shape[0])
    else:                                                  # (uploaded as bytes: every sample type the same way)
        host = cat if packed else (np.concatenate(caps) if caps else np.zeros((0, 2), npdt))
        total = int(host.shape[0])
        iq = torch.from_numpy(np.ascontiguousarray(host).reshape(-1).view(np.uint8)).to(pipe.device)
    n_meta = 4 * k + 1
    meta_bytes = (8 * n_meta + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
    block = C.sizeof(_lib.NoiseResult)
    # nothing below waits for the stream: the staging buffer is one no earlier call's upload is still reading (_idle_stage)
    stage = _idle_stage(torch, pool, "batch_costas_stages", meta_bytes + block * k)
    view = stage.numpy()
    meta = view[:8 * n_meta].view(np.int64)
    meta[:k + 1] = starts
    meta[k + 1:] = plan
    if noise is not None:                                  # a result block per capture as k_batch_noise leaves it for flag 1: noise_f32 and its fp32 square
        view[meta_bytes:meta_bytes + block * k] = 0
        blocks = (_lib.NoiseResult * k).from_address(stage.data_ptr() + meta_bytes)
        for r, value in zip(blocks, noise):
            f = np.float32(value)
            r.noise, r.noise_f32, r.noise_sqrd, r.flag = float(value), float(f), float(f * f), 1
    in_bytes = meta_bytes + (block * k if noise is not None else 0)
    stream = torch.cuda.current_stream(pipe.device)
    pipe.ctx.set_stream(stream.cuda_stream)
    dev_in = torch.empty(max(in_bytes, 8), dtype=torch.uint8, device=pipe.device)      # (of this call alone: the launch before may still read its own)
    dev_in.copy_(stage[:max(in_bytes, 8)], non_blocking=True)
    _stage_in_flight(torch, pool, "batch_costas_stages", stage, stream)
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device)
    _lib.check(lib.urhgpu_batch_costas_dev(pipe.ctx.handle, C.c_void_p(iq.data_ptr()), total, C.c_void_p(dev_in.data_ptr()),
                                           C.c_void_p(dev_in.data_ptr() + 8 * (k + 1)), k, C.byref(cp),
                                           C.c_void_p(dev_in.data_ptr() + meta_bytes) if noise is not None else None, C.c_void_p(qad.data_ptr())))
    return qad[:total], starts                             # (queued on torch's current stream: the samples' memory is not reused before the launch has run)


def check_batch_dc_options(p, message_length_divisor=None, **options):
    """iq_to_bits_batch_dc takes the options of its signature alone: anything else is a TypeError, a divisor below 1 and a modulation no batch
    demodulates a ValueError (host arithmetic: no GPU needed)"""
    for name in options:
        raise TypeError(f"iq_to_bits_batch_dc() got an unexpected keyword argument '{name}'")
    if is_psk(p):
        check_batch_psk_options(p)
    else:
        check_batch_options(p)
    if message_length_divisor is not None and not 1 <= int(message_length_divisor) <= 1 << 30:
        raise ValueError("message_length_divisor must be at least 1 (and at most 2 ** 30)")


def _dc_correct(pipe, pool, caps, lengths, npdt, on_device, cat=None, starts_in=None):
    """urhgpu_batch_dc_correct_dev on the captures `caps` (numpy arrays or device tensors, as _batch_input hands them out), or on cat with
    starts_in where a packed buffer is taken whole: one upload -- starts, plan and, for host captures, every sample --, two launches, nothing
    waited for.  Host captures are corrected in place in their upload, a concatenation made here in place too; a caller's device tensor is
    read and the result written into a buffer of the same geometry.  Returns (iq_cat (total, 2) on the device, starts, the means as a device
    tensor of 2 K float32 / float64)."""
    from .iq_array import _torch_dtype_for
    from .pipeline import DemodParams
    from .signal_functions import dtype_code
    torch, lib = pipe.torch, _lib.load()
    npdt = np.dtype(npdt)
    k = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)            # (of the plan only the launch order is read)
    plan, _, _ = batch_plan(lengths, p.to_c(npdt))
    if cat is not None:
        starts, total = np.asarray(starts_in, dtype=np.int64), int(len(cat))
    else:
        starts = np.zeros(k + 1, np.int64)
        np.cumsum(lengths, out=starts[1:])
        total = int(starts[-1])
    item = 2 * npdt.itemsize
    n_meta = 4 * k + 1
    meta_bytes = (8 * n_meta + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
    in_bytes = meta_bytes + (0 if on_device else total * item)
    # nothing below waits for the stream: the staging buffer is one no earlier call's upload is still reading (_idle_stage)
    stage = _idle_stage(torch, pool, "batch_dc_stages", in_bytes)
    view = stage.numpy()
    meta = view[:8 * n_meta].view(np.int64)
    meta[:k + 1] = starts
    meta[k + 1:] = plan
    if not on_device:
        if cat is not None:
            view[meta_bytes:in_bytes] = cat.reshape(-1).view(np.uint8)
        else:
            for a, s in zip(caps, starts[:-1]):
                if len(a):
                    view[meta_bytes + int(s) * item: meta_bytes + (int(s) + len(a)) * item] = a.reshape(-1).view(np.uint8)
    stream = torch.cuda.current_stream(pipe.device)
    pipe.ctx.set_stream(stream.cuda_stream)
    dev_in = torch.empty(in_bytes, dtype=torch.uint8, device=pipe.device)       # (of this call alone: the result of a host batch is a view of it)
    dev_in.copy_(stage[:in_bytes], non_blocking=True)                            # THE upload
    _stage_in_flight(torch, pool, "batch_dc_stages", stage, stream)
    tdt = _torch_dtype_for(npdt)
    if not on_device:
        src = out = dev_in[meta_bytes:in_bytes].view(tdt).reshape(total, 2)
    else:
        src = cat if cat is not None else (torch.cat(caps) if caps else torch.empty((0, 2), dtype=tdt, device=pipe.device))
        mine = cat is None or not src.is_contiguous()                            # a tensor made here may be corrected where it lies
        src = src.contiguous()
        if src.data_ptr() % 16:                                                  # (a view that starts off a 16-byte boundary)
            src, mine = src.clone(), True
        out = src if mine else torch.empty_like(src)
    d_mean = torch.empty(max(2 * k, 1), dtype=torch.float32 if npdt == np.float32 else torch.float64, device=pipe.device)
    _lib.check(lib.urhgpu_batch_dc_correct_dev(pipe.ctx.handle, C.c_void_p(src.data_ptr()), total, dtype_code(npdt), C.c_void_p(dev_in.data_ptr()),
                                               C.c_void_p(dev_in.data_ptr() + 8 * (k + 1)), k, C.c_void_p(out.data_ptr()), C.c_void_p(d_mean.data_ptr())))
    return out, starts, d_mean[:2 * k]     # (queued on torch's current stream: no memory of this call is reused before the launches have run)


def dc_correct_batch(pipe, captures, want_means=False, _pool=None):
    """DevicePipeline.dc_correct_batch (see there)"""
    pool = pipe._pinned if _pool is None else _pool
    caps, on_device, packed, cat, starts_in, npdt, lengths = _batch_input(pipe, captures)
    iq, starts, d_mean = _dc_correct(pipe, pool, caps, lengths, npdt, on_device, cat if packed else None, starts_in if packed else None)
    if want_means:
        return iq, starts, d_mean.cpu().numpy().reshape(len(lengths), 2)
    return iq, starts


def iq_to_bits_batch_dc(pipe, captures, p, auto_noise=False, auto_center=False, center_max_size=None, message_length_divisor=None, want_qad=False,
                        cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_dc (see there)"""
    check_batch_dc_options(p, message_length_divisor, **options)
    center = {"max_size": center_max_size, "cap_tie": _cap_tie} if auto_center else None
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, bool(auto_noise), center=center,
                  records=None if message_length_divisor is None else int(message_length_divisor), psk=is_psk(p), dc=True)


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


def detect_centers(pipe, captures, max_size=None, return_flags=False, _cap_tie=None, _pool=None):
    """DevicePipeline.detect_centers (see there)"""
    from .pipeline import DemodParams
    torch, lib = pipe.torch, _lib.load()
    qad, starts = _qad_batch_input(pipe, captures)
    k = len(starts) - 1
    pool = pipe._pinned if _pool is None else _pool
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)            # (the chain reads the demodulated signal alone)
    cp = p.to_c(np.float32)
    pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
    d_start = pipe._buf("batch:center_starts", (k + 1,), torch.int64)
    d_start.copy_(torch.from_numpy(starts), non_blocking=False)
    total = int(qad.shape[0])
    scratch, scratch_bytes, _, _, res, tie, cap_tie = _center_buffers(pipe, k, total, 2, _cap_tie)
    _lib.check(lib.urhgpu_batch_center_dev(pipe.ctx.handle, C.c_void_p(qad.data_ptr()), total, C.c_void_p(d_start.data_ptr()), k, C.byref(cp),
                                           -1 if max_size is None else int(max_size), None, C.c_void_p(scratch.data_ptr()), scratch_bytes, None, 0,
                                           C.c_void_p(res.data_ptr()), k + 1, C.c_void_p(tie.data_ptr()), cap_tie))
    blocks, counts = _fetch_centers(pipe, pool, res, k, tie, cap_tie)
    lengths = np.diff(starts)
    centers, flags, _ = _settle_centers(pipe, blocks, counts, k, qad, starts, lambda i: int(lengths[i]), max_size)
    return (centers, flags) if return_flags else centers


def qad_to_bits_batch(pipe, captures, p, centers=None, cap_rows=None, _pool=None):
    """DevicePipeline.qad_to_bits_batch (see there)"""
    check_batch_options(p)
    qad, starts = _qad_batch_input(pipe, captures)
    k = len(starts) - 1
    if centers is not None and len(centers) != k:
        raise ValueError("centers holds one entry per capture (a float, or None for p.center)")
    pool = pipe._pinned if _pool is None else _pool
    items = _walk_qad(pipe, pool, qad, starts, p, None if centers is None else center_thresholds(p, centers), cap_rows)
    qads = [qad[int(a):int(b)] for a, b in zip(starts[:-1], starts[1:])]

    def rerun(j, rows):
        one = qad_to_bits_batch(pipe, (qads[j].contiguous(), [0, qads[j].shape[0]]), p, None if centers is None else [centers[j]], int(rows), _pool={})
        return one[0], qads[j]
    return BatchBits(items, p, np.diff(starts), qads, rerun, centers=None if centers is None else list(centers))


def _batch_input(pipe, captures):
    """the three input forms of a batch -- a list of (N, 2) / complex64 numpy arrays, a list of device tensors, (iq_cat, starts) with a numpy
    array or a device tensor -- as (captures, on the device?, given packed?, iq_cat, starts, numpy sample type, lengths)"""
    torch = pipe.torch
    from .pipeline import _torch_dtype
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
    lengths = [int(c.shape[0]) for c in caps]
    return caps, on_device, packed, cat, starts_in, npdt, lengths


def _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, auto_noise, center=None, records=None, psk=False, dc=False):
    """iq_to_bits_batch, iq_to_bits_batch_auto, iq_to_bits_batch_center, iq_to_bits_batch_records (records: the message_length_divisor),
    iq_to_bits_batch_psk (psk: any combination of the others' options) and iq_to_bits_batch_dc (dc: any of them over the corrected captures):
    the input forms, the routing by length, the result sequence"""
    torch = pipe.torch
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    pool = pipe._pinned if _pool is None else _pool
    caps, on_device, packed, cat, starts_in, npdt, lengths = _batch_input(pipe, captures)
    short, long_ = route(lengths, long_from)
    items = [None] * len(caps)
    qads = [None] * len(caps) if want_qad else None
    noise, flags = ([0.0] * len(caps), [1] * len(caps)) if auto_noise else (None, None)
    centers, cflags = ([None] * len(caps), [0] * len(caps)) if center is not None else (None, None)
    means = np.full((len(caps), 2), np.nan, np.float32 if npdt == np.float32 else np.float64) if dc else None

    # the short ones: one batch
    sub = [caps[i] for i in short]
    sub_len = [lengths[i] for i in short]
    d_mean = None
    if dc:
        # two launches in front: the short captures corrected in ONE buffer on the device (host captures: in their upload), which the batch
        # then reads through its device_iq form
        whole = packed and len(long_) == 0
        dev_cat, dev_starts, d_mean = _dc_correct(pipe, pool, sub, sub_len, npdt, on_device, cat if whole else None, starts_in if whole else None)
        got, qad, src, starts, found, cfound = _run_batch(pipe, None, sub_len, npdt, p, want_qad, cap_rows, pool, device_iq=dev_cat, device_starts=dev_starts,
                                                          auto_noise=auto_noise, center=center, records=records, psk=psk)
    elif on_device:
        if packed and len(long_) == 0 and cat.is_contiguous():
            dev_cat, dev_starts = cat, starts_in
        else:
            dev_cat = torch.cat(sub) if sub else torch.empty((0, 2), dtype=caps[0].dtype if caps else torch.float32, device=pipe.device)
            dev_starts = None
        dev_cat = dev_cat.contiguous()
        got, qad, src, starts, found, cfound = _run_batch(pipe, None, sub_len, npdt, p, want_qad, cap_rows, pool, device_iq=dev_cat, device_starts=dev_starts,
                                                          auto_noise=auto_noise, center=center, records=records, psk=psk)
    else:
        got, qad, src, starts, found, cfound = _run_batch(pipe, sub, sub_len, npdt, p, want_qad, cap_rows, pool, auto_noise=auto_noise, center=center,
                                                          records=records, psk=psk)
    if auto_noise == "only":
        return found
    for j, i in enumerate(short):
        items[i] = got[j]
        items[i].seq = int(i)
        if auto_noise:
            noise[i], flags[i] = found[0][j], found[1][j]
        if center is not None:
            centers[i], cflags[i] = cfound[0][j], cfound[1][j]
        if want_qad:
            qads[i] = qad[int(starts[j]):int(starts[j]) + items[i].n_samples]     # (an auto_noise capture that is gated entirely: zeros(2))
    if dc and len(short):
        means[short] = d_mean.cpu().numpy().reshape(-1, 2)       # (the batch's fetch has waited for the stream: this copy waits for nothing)

    # the long ones: an ordinary pass each
    p_pass = replace(p, write_bit_sample_pos=False)
    for i in long_:
        c = caps[i]
        t = c if on_device else torch.from_numpy(c).to(pipe.device)
        if dc:                                             # (the pass keeps its means to itself: they are taken once more for .means)
            from .filter import dc_correct_dev
            means[i] = dc_correct_dev(pipe, t.contiguous(), want_mean=True)[1].cpu().numpy()
        res = pipe.iq_to_bits(t.contiguous(), p_pass, want_qad=want_qad or center is not None, cap_rows=cap_rows if isinstance(cap_rows, int) else None,
                              auto_noise=bool(auto_noise), auto_center=center is not None, center_max_size=center["max_size"] if center else None,
                              msg_records=records is not None, message_length_divisor=records or 1, dc_correction=dc)
        if auto_noise:
            flags[i] = res.noise_flag
            noise[i] = float(res._noise)
            if flags[i] == 0:                              # the reference raises for this capture: nothing to hand out
                continue
        if center is not None:
            centers[i], cflags[i] = res.center, res.center_flag
        h = res.host(pool={})
        h.seq = int(i)
        if records is not None:                            # a copy of the pass's records: its pinned block belongs to the slot
            from .protocol import RECORD_DTYPE
            try:
                h.records = res.records.copy()
            except _lib.UrhGpuError:                       # (a capacity was exceeded: message_data() says so, retry(k) repeats the capture)
                h.records = np.zeros(0, RECORD_DTYPE)
        items[i] = h
        if want_qad:
            qads[i] = res.qad.clone()

    def rerun(k, rows):
        """capture k alone with `rows` rows of capacity, results in pinned memory of their own"""
        c = caps[k]
        t = c if on_device else torch.from_numpy(c).to(pipe.device)
        if dc:                                             # (corrected again, alone through the same entry point, with the options of the batch)
            one = iq_to_bits_batch_dc(pipe, [t.contiguous()], p, bool(auto_noise), center is not None, center["max_size"] if center else None, records,
                                      want_qad, int(rows), long_from, _pool={}, _cap_tie=center.get("cap_tie") if center else None)
        elif psk:                                          # (alone through the same entry point, with the options of the batch)
            one = iq_to_bits_batch_psk(pipe, [t.contiguous()], p, bool(auto_noise), center is not None, center["max_size"] if center else None, records,
                                       want_qad, int(rows), long_from, _pool={}, _cap_tie=center.get("cap_tie") if center else None)
        elif records is not None:                          # (alone through the same entry point, records included)
            one = iq_to_bits_batch_records(pipe, [t.contiguous()], p, records, bool(auto_noise), center is not None, center["max_size"] if center else None,
                                           want_qad, int(rows), long_from, _pool={}, _cap_tie=center.get("cap_tie") if center else None)
        elif center is not None:                           # (alone through the same entry point: it detects the same threshold and center)
            one = iq_to_bits_batch_center(pipe, [t.contiguous()], p, auto_noise=bool(auto_noise), center_max_size=center["max_size"], want_qad=want_qad,
                                          cap_rows=int(rows), long_from=long_from, _pool={}, _cap_tie=center.get("cap_tie"))
        elif auto_noise:                                   # (alone through the same entry point: it detects the same threshold)
            one = iq_to_bits_batch_auto(pipe, [t.contiguous()], p, want_qad=want_qad, cap_rows=int(rows), long_from=long_from, _pool={})
        else:
            one = iq_to_bits_batch(pipe, [t.contiguous()], p, want_qad=want_qad, cap_rows=int(rows), long_from=long_from, _pool={})
        return one[0], (one.qad(0) if want_qad else None)

    return BatchBits(items, p, lengths, qads, rerun, noise, flags, centers, cflags, means)


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


# ---- the estimate of a session: every capture's parameters (include/urhgpu.h "a batch of captures: message ranges per capture") ------------
# messages whose centers and plateau decisions go through one native call: urhgpu_msg_estimate refuses (URHGPU_ERR_UNSUPPORTED) more than
# 64 MiB of histogram pool, 4096 counters of 4 bytes per message
MSG_GROUP = 4096

_ESTIMATE_MODULATIONS = ("OOK", "ASK", "FSK", "PSK")
# estimators.estimate_dev agrees with the reference on these sample types here (tests/test_gpu_parity.py); uint8 and uint16 are not covered
# by such a test, so a session of them is refused instead of estimated unchecked
ESTIMATE_SAMPLE_TYPES = (np.float32, np.int8, np.int16)


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


def check_estimate_options(k, npdt, noise, modulation):
    """(noise per capture, modulation per capture) of estimate_batch, or ValueError with a sentence (host arithmetic: no GPU needed)"""
    if np.dtype(npdt) not in [np.dtype(t) for t in ESTIMATE_SAMPLE_TYPES]:
        raise ValueError(f"estimate_batch takes float32, int8 and int16 captures, not {np.dtype(npdt).name}: estimate_dev is not verified against the "
                         "reference on that sample type")

    def check_mod(m):
        if m is not None and m not in _ESTIMATE_MODULATIONS:
            raise ValueError("Unsupported Modulation")           # (what the reference raises, AutoInterpretation.py:394)
    mods = per_capture(modulation, k, "modulation", check_mod)
    noises = [None if v is None else float(v) for v in per_capture(noise, k, "noise")]
    return noises, mods


class BatchEstimates:
    """The results of estimate_batch: a sequence with one entry per capture in the order given -- the dict estimators.estimate_dev returns
    (modulation_type, bit_length, center, tolerance, noise), or None.  A capture for which the reference raises (detect_noise_level on a
    capture whose magnitudes hold a NaN or an infinity) raises the same exception where it is handed out, as BatchBits does; the others are
    handed out."""

    def __init__(self, items, errors, lengths):
        self._items, self._errors = list(items), list(errors)
        self.lengths = [int(n) for n in lengths]

    def __len__(self):
        return len(self._items)

    def _hand_out(self, k):
        if self._errors[k] is not None:
            raise self._errors[k]
        return self._items[k]

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self._hand_out(i) for i in range(*k.indices(len(self._items)))]
        return self._hand_out(range(len(self._items))[k])

    def __iter__(self):
        return (self._hand_out(k) for k in range(len(self._items)))


class _Session:
    """the short captures of a session on the device: the samples back to back, their starts, the plan's launch order and the regions of
    the segmentation, uploaded with ONE copy"""

    def __init__(self, pipe, pool, caps, lengths, npdt, device_iq=None, device_starts=None):
        torch = self.torch = pipe.torch
        from .pipeline import DemodParams
        self.pipe, self.pool, self.npdt = pipe, pool, np.dtype(npdt)
        k = self.k = len(lengths)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False)            # (of the plan only the launch order is read)
        plan, _, _ = batch_plan(self.lengths, p.to_c(self.npdt))
        starts = np.zeros(k + 1, np.int64)
        np.cumsum(self.lengths, out=starts[1:])
        if device_starts is not None:
            starts = np.asarray(device_starts, dtype=np.int64)
        self.starts = starts
        self.total = int(starts[-1]) if device_iq is None else int(device_iq.shape[0])
        self.seg_caps = self.lengths // 20 + 1                                      # urhgpu_batch_segments_capacity
        regions = np.zeros(k + 1, np.int64)
        np.cumsum(self.seg_caps, out=regions[1:])
        self.cap_seg = int(regions[-1])
        item = 2 * self.npdt.itemsize
        n_meta = 5 * k + 1
        self.meta_bytes = (8 * n_meta + _META_ALIGN - 1) // _META_ALIGN * _META_ALIGN
        in_bytes = self.meta_bytes + (self.total * item if device_iq is None else 0)
        stage = _pinned(torch, pool, "estimate_stage", in_bytes)
        view = stage.numpy()
        meta = view[:8 * n_meta].view(np.int64)
        meta[:k + 1] = starts
        meta[k + 1:4 * k + 1] = plan
        meta[4 * k + 1:] = regions[:-1]
        if device_iq is None:
            for a, s in zip(caps, starts[:-1]):
                if len(a):
                    view[self.meta_bytes + int(s) * item: self.meta_bytes + (int(s) + len(a)) * item] = a.reshape(-1).view(np.uint8)
        pipe.ctx.set_stream(torch.cuda.current_stream(pipe.device).cuda_stream)
        self.dev_in = pipe._buf("estimate:in", (max(in_bytes, 16),), torch.uint8)
        self.dev_in[:in_bytes].copy_(stage[:in_bytes], non_blocking=True)          # THE upload: starts, plan, regions and every sample in one copy
        self.d_start = self.dev_in.data_ptr()
        self.d_plan = self.d_start + 8 * (k + 1)
        self.d_region = self.d_start + 8 * (4 * k + 1)
        if device_iq is None:
            from .iq_array import _torch_dtype_for
            self.iq = self.dev_in[self.meta_bytes:self.meta_bytes + self.total * item].view(_torch_dtype_for(self.npdt)).reshape(self.total, 2)
        else:
            self.iq = device_iq
        self.cp = p.to_c(self.npdt)

    def upload_noise(self, noise):
        """the captures' thresholds as the kernels read them, ONE copy: float[k] for the segmentation ((float)noise, afp_demod's and
        segment_messages_from_magnitudes' `float` argument) and urhgpu_noise_result[k] for the demodulation -- flag 1 and the DETECTED value
        whatever Signal.max_magnitude says: the estimate never asks (k_batch_noise's own blocks carry the configured threshold for flag 2)"""
        torch, k = self.torch, self.k
        thr_bytes = (4 * k + 15) // 16 * 16
        nbytes = thr_bytes + C.sizeof(_lib.NoiseResult) * max(k, 1)
        stage = _pinned(torch, self.pool, "estimate_noise_stage", nbytes)
        view = stage.numpy()
        view[:nbytes] = 0
        thr = view[:4 * k].view(np.float32)
        with np.errstate(all="ignore"):
            thr[:] = np.asarray(noise, dtype=np.float64).astype(np.float32)
            sq = thr * thr                                                          # an fp32 multiply
        blocks = (_lib.NoiseResult * max(k, 1)).from_address(stage.data_ptr() + thr_bytes)
        for i in range(k):
            blocks[i].noise, blocks[i].noise_f32, blocks[i].noise_sqrd, blocks[i].flag = float(noise[i]), float(thr[i]), float(sq[i]), 1
        dev = self.pipe._buf("estimate:noise_in", (nbytes,), torch.uint8)
        dev.copy_(stage[:nbytes], non_blocking=True)
        self.d_thr, self.d_noise_blocks = dev.data_ptr(), dev.data_ptr() + thr_bytes

    def detect_noise(self):
        """AutoInterpretation.detect_noise_level of every capture: k_batch_noise and one read of the K blocks -> (values, flags)"""
        torch, k, lib = self.torch, self.k, _lib.load()
        d_noise = self.pipe._buf("batch:noise", (C.sizeof(_lib.NoiseResult) * max(k, 1),), torch.uint8)
        _lib.check(lib.urhgpu_batch_noise_dev(self.pipe.ctx.handle, C.c_void_p(self.iq.data_ptr()), self.total, C.c_void_p(self.d_start), C.c_void_p(self.d_plan),
                                              k, C.byref(self.cp), C.c_void_p(d_noise.data_ptr())))
        h = _pinned(torch, self.pool, "batch_noise", C.sizeof(_lib.NoiseResult) * max(k, 1))
        _lib.check(lib.urhgpu_batch_noise_fetch(self.pipe.ctx.handle, C.c_void_p(d_noise.data_ptr()), k, C.c_void_p(h.data_ptr())))
        blocks = (_lib.NoiseResult * k).from_address(h.data_ptr())
        return [float(r.noise) for r in blocks], [int(r.flag) for r in blocks]

    def segments(self):
        """urhgpu_batch_segments_dev and its fetch with the thresholds uploaded last: three launches and two copies -> one int64 (n, 2) array
        per capture, relative to the capture's first sample"""
        torch, k, lib, pipe = self.torch, self.k, _lib.load(), self.pipe
        cap = max(self.cap_seg, 1)
        seg = pipe._buf("estimate:seg", (2 * cap,), torch.int64)
        out = pipe._buf("estimate:seg_out", (2 * cap,), torch.int64)
        counts = pipe._buf("estimate:seg_counts", (max(k, 1),), torch.int64)
        d_dir = pipe._buf("estimate:seg_dir", (k + 1,), torch.int64)
        from .signal_functions import dtype_code
        _lib.check(lib.urhgpu_batch_segments_dev(pipe.ctx.handle, C.c_void_p(self.iq.data_ptr()), dtype_code(self.npdt), self.total, C.c_void_p(self.d_start),
                                                 C.c_void_p(self.d_plan), k, C.c_void_p(self.d_thr), C.c_void_p(self.d_region), C.c_void_p(seg.data_ptr()),
                                                 self.cap_seg, C.c_void_p(counts.data_ptr()), C.c_void_p(d_dir.data_ptr()), C.c_void_p(out.data_ptr()), self.cap_seg))
        h_dir = _pinned(torch, self.pool, "estimate_seg_dir", 8 * (k + 1))
        h_out = _pinned(torch, self.pool, "estimate_seg_out", 16 * cap)
        m = C.c_int64(0)
        _lib.check(lib.urhgpu_batch_segments_fetch(pipe.ctx.handle, C.c_void_p(d_dir.data_ptr()), k, C.c_void_p(out.data_ptr()), C.c_void_p(h_dir.data_ptr()),
                                                   C.c_void_p(h_out.data_ptr()), cap, C.byref(m)))
        offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
        pairs = h_out.numpy()[:16 * int(m.value)].view(np.int64).reshape(-1, 2).copy()
        return [pairs[int(offs[i]):int(offs[i + 1])] for i in range(k)]

    def demod(self, mod):
        """urhgpu_batch_demod_dev: afp_demod(capture, its noise, mod) of every capture into one float32 device tensor -- one launch"""
        from .pipeline import DemodParams
        torch, pipe = self.torch, self.pipe
        cp = DemodParams(mod, 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, False).to_c(self.npdt)
        qad = pipe._buf("estimate:qad_" + mod, (max(self.total, 1),), torch.float32)
        _lib.check(_lib.load().urhgpu_batch_demod_dev(pipe.ctx.handle, C.c_void_p(self.iq.data_ptr()), self.total, C.c_void_p(self.d_start), C.c_void_p(self.d_plan),
                                                      self.k, C.byref(cp), C.c_void_p(self.d_noise_blocks), C.c_void_p(qad.data_ptr())))
        return qad


def _session(pipe, pool, caps, lengths, npdt, on_device, packed, cat, starts_in, whole):
    """the captures `caps` as a _Session; a packed device tensor that is taken whole is read where it lies"""
    torch = pipe.torch
    if not on_device:
        return _Session(pipe, pool, caps, lengths, npdt)
    if packed and whole and cat.is_contiguous():
        return _Session(pipe, pool, None, lengths, npdt, device_iq=cat, device_starts=starts_in)
    from .iq_array import _torch_dtype_for
    dev_cat = torch.cat(caps) if caps else torch.empty((0, 2), dtype=_torch_dtype_for(npdt), device=pipe.device)
    return _Session(pipe, pool, None, lengths, npdt, device_iq=dev_cat.contiguous())


def segment_messages_batch(pipe, captures, noise, _pool=None):
    """DevicePipeline.segment_messages_batch (see there)"""
    pool = pipe._pinned if _pool is None else _pool
    caps, on_device, packed, cat, starts_in, npdt, lengths = _batch_input(pipe, captures)
    noises = [float(v) for v in per_capture(noise, len(caps), "noise")]
    s = _session(pipe, pool, caps, lengths, npdt, on_device, packed, cat, starts_in, True)
    s.upload_noise(noises)
    return s.segments()


def estimate_batch(pipe, captures, noise=None, modulation=None, long_from=None, _pool=None):
    """DevicePipeline.estimate_batch (see there)"""
    from . import estimators as E
    from .pipeline import raise_noise_error
    torch = pipe.torch
    pool = pipe._pinned if _pool is None else _pool
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    caps, on_device, packed, cat, starts_in, npdt, lengths = _batch_input(pipe, captures)
    k_all = len(caps)
    noises, mods = check_estimate_options(k_all, npdt, noise, modulation)
    items, errors = [None] * k_all, [None] * k_all

    def alone(i):
        """capture i through estimate_dev: a long capture, or PSK -- the estimate does not pool PSK captures through k_batch_costas"""
        c = caps[i]
        t = c if on_device else torch.from_numpy(c).to(pipe.device)
        try:
            items[i] = E.estimate_dev(pipe, t.contiguous(), noise=noises[i], modulation=mods[i])
        except (ValueError, OverflowError) as e:              # what the reference raises for this capture: raised where it is handed out
            errors[i] = e

    by_length, long_ = route(lengths, long_from)
    short = [int(i) for i in by_length if mods[i] != "PSK"]
    for i in sorted([int(i) for i in long_] + [int(i) for i in by_length if mods[i] == "PSK"]):
        alone(i)
    k = len(short)
    if k == 0:
        return BatchEstimates(items, errors, lengths)
    s = _session(pipe, pool, [caps[i] for i in short], [lengths[i] for i in short], npdt, on_device, packed, cat, starts_in, k == k_all)

    # 1. noise: detected per capture (one launch, one read), or given
    value = [noises[i] for i in short]
    if any(v is None for v in value):
        found, flags = s.detect_noise()
        for j in range(k):
            if value[j] is None:
                value[j] = found[j]
                if flags[j] == 0:                                 # math.ceil of a NaN / an infinity: the reference raises
                    try:
                        raise_noise_error(found[j])
                    except (ValueError, OverflowError) as e:
                        errors[short[j]] = e
                    value[j] = float("nan")                       # (nothing is above a NaN: no segment, no message)
    s.upload_noise(value)

    # 2. segmentation; 3. the OOK merge per capture on the host (a short capture has a few dozen pulses)
    segs = s.segments()
    live = [j for j in range(k) if errors[short[j]] is None and len(segs[j])]

    # 4. the modulation vote: ONE call over the first 100 ranges of every capture that needs it
    mod_of = [mods[i] for i in short]
    need = [j for j in live if mod_of[j] is None]
    if need:
        ranges = np.concatenate([segs[j][:100] + s.starts[j] for j in need])
        labels = E.detect_modulation_dev(pipe, s.iq, ranges)      # (an integer session: iq_array.convert_to once, inside)
        at = 0
        for j in need:
            n = min(len(segs[j]), 100)
            mod_of[j] = E.most_common_label(labels[at:at + n])
            at += n
    for j in live:
        if mod_of[j] == "PSK":                                    # detected: alone, as estimate_dev detects and estimates it
            alone(short[j])
    msgs = {j: (E.merge_message_segments_for_ook(segs[j]) if mod_of[j] == "OOK" else segs[j]) for j in live if mod_of[j] in ("OOK", "ASK", "FSK")}

    # 5. demodulation, once per modulation group present; 6. the decisions of ALL messages of a group, pooled as global ranges, in chunks
    # that fit the histogram pool; then the votes per capture
    for group in (("OOK", "ASK"), ("FSK",)):
        members = [j for j in sorted(msgs) if mod_of[j] in group]
        if not members:
            continue
        qad = s.demod("ASK" if group[0] == "OOK" else "FSK")
        pooled = np.concatenate([msgs[j] + s.starts[j] for j in members]).astype(np.int64)
        parts = [E.message_decisions(pipe, qad, pooled[a:a + MSG_GROUP]) for a in range(0, len(pooled), MSG_GROUP)]
        center_of, tol_of, len_of = (np.concatenate([p[i] for p in parts]) for i in range(3))
        at = 0
        for j in members:
            n = len(msgs[j])
            noise_j = noises[short[j]] if noises[short[j]] is not None else value[j]
            items[short[j]] = E.vote_on_messages(mod_of[j], noise_j, center_of[at:at + n], tol_of[at:at + n], len_of[at:at + n])
            at += n
    return BatchEstimates(items, errors, lengths)
