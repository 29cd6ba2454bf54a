"""The batch itself: the short captures in one pass of launches, the long ones a pass each, the result sequence; the entry points."""
import ctypes as C
from collections import namedtuple
from dataclasses import replace

import numpy as np

from .. import _lib
from .center import _center_buffers, center_thresholds, fetch_and_settle
from .psk_dc import _dc_correct
from .inputs import LONG_FROM_DEFAULT, _batch_input, _qad_batch_input, back_to_back, route
from .options import BatchOptions, as_fsk, check_batch_auto_options, check_batch_center_options, check_batch_dc_options, check_batch_options
from .options import check_batch_psk_options, check_batch_records_options, is_psk
from .staging import _pinned, batch_plan, captures_at, detect_noise, noise_buffer, order_params, read_noise_blocks, upload
from .walk import RecordSource, _fetch_blobs, _fetch_records, _queue_records, _walk_qad, items_from_blobs, walk_buffers


class CaptureSequence:
    """a result sequence, one entry per capture in the order given: _hand_out(k) is entry k, or raises what the reference raises for that capture"""

    def __len__(self):
        return len(self._items)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self._hand_out(i) for i in range(*k.indices(len(self._items)))]      # (a slice gives a list)
        return self._hand_out(range(len(self._items))[k])

    def __iter__(self):
        return (self._hand_out(k) for k in range(len(self._items)))


class BatchBits(CaptureSequence):
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

    def _hand_out(self, k):
        if self.noise_flags is not None and self.noise_flags[k] == 0:
            from ..pipeline import raise_noise_error
            raise_noise_error(self.noise[k])               # what detect_noise_level raises for this capture; the others are handed out
        return self._items[k]

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


# the short captures of a batch on the device: the Upload, where the samples lie, their starts, the plan and its two sizes
Staged = namedtuple("Staged", "up d_iq total starts plan work_bytes blob_cap")
# what _run_batch hands back: the HostBits, the demodulated buffer (or None), the starts in it, (noise values, flags), (centers, flags), the input
Ran = namedtuple("Ran", "items qad starts noise centers dev_in")


def _stage_batch(pipe, pool, caps, lengths, npdt, cp_plan, cap_rows, device_iq=None, device_starts=None) -> Staged:
    """the plan, and THE upload of a batch: starts, plan and -- for caps, numpy arrays -- every sample in one copy; device_iq: a device tensor
    that holds the captures already, back to back or at device_starts.  The device buffer is a tensor of this call alone."""
    torch = pipe.torch
    plan, work_bytes, blob_cap = batch_plan(lengths, cp_plan, cap_rows)
    starts = back_to_back(lengths) if device_starts is None else np.asarray(device_starts, dtype=np.int64)
    total = int(starts[-1]) if device_iq is None else int(device_iq.shape[0])
    item = 2 * np.dtype(npdt).itemsize
    up = upload(pipe, lambda n: _pinned(torch, pool, "batch_stage", n), lambda n: torch.empty(n, dtype=torch.uint8, device=pipe.device), starts, plan,
                payload_bytes=total * item if device_iq is None else 0, fill=captures_at(caps, starts, item) if device_iq is None else None)
    return Staged(up, up.d_payload if device_iq is None else device_iq.data_ptr(), total, starts, plan, work_bytes, blob_cap)


def _run_batch(pipe, caps, lengths, npdt, p, want_qad, cap_rows, pool, o, device_iq=None, device_starts=None) -> Ran:
    """the short captures of a batch through the three launches.  caps: numpy arrays (packed and uploaded here, one copy), or device_iq (a
    device tensor that holds them back to back) with device_starts.  o, the BatchOptions: auto_noise -- one launch more, every capture gated
    with the threshold detected for it, and one more read, of the K result blocks; center -- every capture sliced with its own center, the
    centers the device left to the host settled and those captures sliced again by ONE more call; records -- the records of all captures
    queued behind the walk (before anything reuses the work buffer) and fetched with one copy, those of a second slicing the same way; psk --
    a Costas loop per capture (one launch, into the qad buffer) and the walk from there; the plan, the walk and the records then take the
    parameters recoded as FSK (as_fsk)."""
    torch, lib = pipe.torch, _lib.load()
    k = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    cp = p.to_c(npdt)
    cp.write_bit_sample_pos = 0
    cp_walk = cp
    if o.psk:
        cp_walk = as_fsk(p).to_c(npdt)
        cp_walk.write_bit_sample_pos = 0
    s = _stage_batch(pipe, pool, caps, lengths, npdt, cp_walk, cap_rows, device_iq, device_starts)
    starts, total = s.starts, s.total
    d_noise = noise_buffer(pipe, k) if o.auto_noise else None
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device) if (want_qad or o.center or o.psk) else None
    bufs = walk_buffers(pipe, k, s.work_bytes, s.blob_cap)
    args = (pipe.ctx.handle, C.c_void_p(s.d_iq), total, C.c_void_p(s.up.d_start), C.c_void_p(s.up.d_plan), k, C.byref(cp))
    out = (C.c_void_p(qad.data_ptr()) if qad is not None else None, C.c_void_p(bufs.work.data_ptr()), s.work_bytes, C.c_void_p(bufs.counts.data_ptr()),
           C.c_void_p(bufs.d_dir.data_ptr()), C.c_void_p(bufs.blob.data_ptr()), s.blob_cap)
    noise_out = C.c_void_p(d_noise.data_ptr()) if o.auto_noise else None
    cb = None
    if o.center:
        cb = _center_buffers(pipe, k, total, 1 << p.bits_per_symbol, o.cap_tie)
        max_size = -1 if o.max_size is None else int(o.max_size)
        chain = (C.c_void_p(cb.scratch.data_ptr()), cb.scratch_bytes, C.c_void_p(cb.thr.data_ptr()), cb.cap_thr, C.c_void_p(cb.res.data_ptr()), k + 1,
                 C.c_void_p(cb.tie.data_ptr()), cb.cap_tie)
        if o.psk:
            _lib.check(lib.urhgpu_iq_to_bits_batch_psk_dev(*args, int(o.auto_noise), 1, max_size, *out, noise_out, *chain))
        else:
            _lib.check(lib.urhgpu_iq_to_bits_batch_center_dev(*args, int(o.auto_noise), max_size, *out, noise_out, *chain))
    elif o.psk:
        _lib.check(lib.urhgpu_iq_to_bits_batch_psk_dev(*args, int(o.auto_noise), 0, -1, *out, noise_out, None, 0, None, 0, None, 0, None, 0))
    elif o.auto_noise:
        _lib.check(lib.urhgpu_iq_to_bits_batch_auto_dev(*args, *out, noise_out))
    else:
        _lib.check(lib.urhgpu_iq_to_bits_batch_dev(*args, *out))
    rec_src = RecordSource(s.d_iq, total, s.up.d_start, k, cp_walk)
    queued = None if o.records is None else _queue_records(pipe, rec_src, None, s.up.d_plan, k, s.plan, o.records, d_noise, bufs)
    fetched = _fetch_blobs(pipe, pool, bufs.d_dir, k, bufs.blob, bufs.blob_cap)
    noise = read_noise_blocks(pipe, pool, d_noise, k) if o.auto_noise else None
    # (noise flag 2: the reference slices zeros(2), and so did the device)
    n_samples = lengths if noise is None else [2 if flag == 2 else int(n) for n, flag in zip(lengths, noise[1])]
    items = items_from_blobs(fetched, k, p, n_samples, qad, starts)
    if queued is not None:
        _fetch_records(pipe, pool, queued, items)
    found = None
    if o.center:
        n_of = lambda i: items[i].n_samples                                          # noqa: E731
        skip = {i for i in range(k) if noise is not None and noise[1][i] == 0}      # (the reference raises for these: nothing is handed out)
        centers, flags, settled = fetch_and_settle(pipe, pool, cb, qad, starts, n_of, o.max_size, skip)
        if settled:
            # ALL the captures the host has settled a center for, sliced again by ONE call: their demodulated signals gathered back to back
            # (one torch.cat), the thresholds of their centers uploaded with the starts and the plan
            parts = [qad[int(starts[i]):int(starts[i]) + n_of(i)] for i in settled]
            sub = torch.cat(parts) if len(parts) > 1 else parts[0]
            again = _walk_qad(pipe, pool, sub.contiguous(), back_to_back([n_of(i) for i in settled]), p, center_thresholds(p, [centers[i] for i in settled]),
                              cap_rows, tag=":again", records=None if o.records is None else (o.records, rec_src, np.asarray(settled, dtype=np.int64)))
            for i, h in zip(settled, again):
                h.seq = i
                items[i] = h
        found = (centers, flags)
    return Ran(items, qad, starts, noise, found, s.up.dev_in)


def _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, o):
    """every iq_to_bits_batch* entry point behind its checks, with its options as a BatchOptions: the input forms, the routing by length, the
    result sequence"""
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    pool = pipe._pinned if _pool is None else _pool
    given = _batch_input(pipe, captures)
    caps, lengths, n = given.caps, given.lengths, len(given.caps)
    short, long_ = route(lengths, long_from)
    items = [None] * n
    qads = [None] * n if want_qad else None
    noise, flags = ([0.0] * n, [1] * n) if o.auto_noise else (None, None)
    centers, cflags = ([None] * n, [0] * n) if o.center else (None, None)
    means = np.full((n, 2), np.nan, np.float32 if given.npdt == np.float32 else np.float64) if o.dc else None

    # the short ones: one batch -- behind the DC correction's two launches (ONE corrected buffer on the device), from device captures back to back, or
    # from host captures packed into the upload
    dev_cat = dev_starts = d_mean = None
    if o.dc:
        dev_cat, dev_starts, d_mean = _dc_correct(pipe, pool, given, short)
    elif given.on_device:
        dev_cat, dev_starts = given.device_cat(pipe, short)
    got, qad, starts, found, cfound, _ = _run_batch(pipe, None if dev_cat is not None else [caps[i] for i in short], [lengths[i] for i in short], given.npdt, p,
                                                    want_qad, cap_rows, pool, o, dev_cat, dev_starts)
    for j, i in enumerate(short):
        items[i] = got[j]
        items[i].seq = int(i)
        if found is not None:
            noise[i], flags[i] = found[0][j], found[1][j]
        if cfound is not None:
            centers[i], cflags[i] = cfound[0][j], cfound[1][j]
        if want_qad:
            qads[i] = qad[int(starts[j]):int(starts[j]) + items[i].n_samples]     # (an auto_noise capture that is gated entirely: zeros(2))
    if o.dc and len(short):
        means[short] = d_mean.cpu().numpy().reshape(-1, 2)       # (the batch's fetch has waited for the stream: this copy waits for nothing)

    # the long ones: an ordinary pass each
    p_pass = replace(p, write_bit_sample_pos=False)
    for i in long_:
        t = given.tensor(pipe, i)
        if o.dc:                                           # (the pass keeps its means to itself: they are taken once more for .means)
            from ..filter import dc_correct_dev
            means[i] = dc_correct_dev(pipe, t, want_mean=True)[1].cpu().numpy()
        res = pipe.iq_to_bits(t, p_pass, want_qad=want_qad or o.center, cap_rows=cap_rows if isinstance(cap_rows, int) else None,
                              auto_noise=o.auto_noise, auto_center=o.center, center_max_size=o.max_size if o.center else None,
                              msg_records=o.records is not None, message_length_divisor=o.records or 1, dc_correction=o.dc)
        if o.auto_noise:
            flags[i] = res.noise_flag
            noise[i] = float(res._noise)
            if flags[i] == 0:                              # the reference raises for this capture: nothing to hand out
                continue
        if o.center:
            centers[i], cflags[i] = res.center, res.center_flag
        h = res.host(pool={})
        h.seq = int(i)
        if o.records is not None:                          # a copy of the pass's records: its pinned block belongs to the slot
            from ..protocol import RECORD_DTYPE
            try:
                h.records = res.records.copy()
            except _lib.UrhGpuError:                       # (a capacity was exceeded: message_data() says so, retry(k) repeats the capture)
                h.records = np.zeros(0, RECORD_DTYPE)
        items[i] = h
        if want_qad:
            qads[i] = res.qad.clone()

    def rerun(k, rows):
        """capture k alone with `rows` rows of capacity and the options of the batch, results in pinned memory of their own"""
        one = _batch(pipe, [given.tensor(pipe, k)], p, want_qad, int(rows), long_from, {}, o)
        return one[0], (one.qad(0) if want_qad else None)

    return BatchBits(items, p, lengths, qads, rerun, noise, flags, centers, cflags, means)


def _options(auto_noise=False, auto_center=False, center_max_size=None, cap_tie=None, divisor=None, psk=False, dc=False):
    return BatchOptions(bool(auto_noise), bool(auto_center), center_max_size if auto_center else None, cap_tie if auto_center else None,
                        None if divisor is None else int(divisor), psk, dc)


def iq_to_bits_batch(pipe, captures, p, want_qad=False, cap_rows=None, long_from=None, _pool=None, **options):
    """DevicePipeline.iq_to_bits_batch (see there)"""
    check_batch_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, _options())


def iq_to_bits_batch_auto(pipe, captures, p, auto_noise=True, want_qad=False, cap_rows=None, long_from=None, _pool=None, **options):
    """DevicePipeline.iq_to_bits_batch_auto (see there)"""
    check_batch_auto_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, _options(auto_noise))


def iq_to_bits_batch_center(pipe, captures, p, auto_noise=True, center_max_size=None, want_qad=False, cap_rows=None, long_from=None, _pool=None,
                            _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_center (see there)"""
    check_batch_center_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, _options(auto_noise, True, center_max_size, _cap_tie))


def iq_to_bits_batch_records(pipe, captures, p, message_length_divisor=1, auto_noise=False, auto_center=False, center_max_size=None, want_qad=False,
                             cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_records (see there)"""
    check_batch_records_options(p, message_length_divisor, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, _options(auto_noise, auto_center, center_max_size, _cap_tie, message_length_divisor))


def iq_to_bits_batch_psk(pipe, captures, p, auto_noise=False, auto_center=False, center_max_size=None, message_length_divisor=None, want_qad=False,
                         cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_psk (see there)"""
    check_batch_psk_options(p, message_length_divisor, **options)
    o = _options(auto_noise, auto_center, center_max_size, _cap_tie, message_length_divisor, psk=True)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, o)


def iq_to_bits_batch_dc(pipe, captures, p, auto_noise=False, auto_center=False, center_max_size=None, message_length_divisor=None, want_qad=False,
                        cap_rows=None, long_from=None, _pool=None, _cap_tie=None, **options):
    """DevicePipeline.iq_to_bits_batch_dc (see there)"""
    check_batch_dc_options(p, message_length_divisor, **options)
    o = _options(auto_noise, auto_center, center_max_size, _cap_tie, message_length_divisor, psk=is_psk(p), dc=True)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, o)


def detect_noise_levels(pipe, captures):
    """AutoInterpretation.detect_noise_level of every capture of a batch (the three input forms of iq_to_bits_batch): ONE launch and one
    read of the K result blocks, whatever K and the lengths are -- the batch counterpart of estimators.detect_noise_level_dev.  Returns the
    list of thresholds (Python floats; a value that is not below the sample type's max_magnitude is returned as it is); where the reference
    raises for a capture (math.ceil of a NaN / an infinity), so does this."""
    from ..pipeline import raise_noise_error
    given = _batch_input(pipe, captures)
    k = len(given.caps)
    cp = order_params().to_c(given.npdt)                   # (the detection reads the samples and the sample type alone)
    cp.write_bit_sample_pos = 0
    dev_cat, dev_starts = given.device_cat(pipe) if given.on_device else (None, None)
    s = _stage_batch(pipe, pipe._pinned, given.caps, given.lengths, given.npdt, cp, None, dev_cat, dev_starts)
    noise, flags = detect_noise(pipe, pipe._pinned, s.d_iq, s.total, s.up.d_start, s.up.d_plan, k, cp)
    for value, flag in zip(noise, flags):
        if flag == 0:
            raise_noise_error(value)
    return noise


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
