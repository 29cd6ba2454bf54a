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
"""
import ctypes as C
from dataclasses import replace

import numpy as np

from . import _lib
from .host_bits import HostBits
from .signal_functions import mod_code

# a capture of this many samples or more goes through an ordinary pass: the capture length at which a batch's wavefront per capture stops
# beating a pipelined stream's pass per capture -- measured: B / A = 1.39 at 131 072 samples, 1.02 and 0.98 at 196 608 (two runs), 0.98 at 262 144
# (tools/batch_probe.py, profiles/batch_probe.txt; DESIGN.md 7.7e has the table)
LONG_FROM_DEFAULT = 196_608

_NOT_IN_A_BATCH = {
    "auto_center": "a batch slices every capture with p.center: call iq_to_bits(..., auto_center=True) per capture, or a CaptureStream(auto_center=True)",
    "auto_noise": "iq_to_bits_batch gates every capture with p.noise_threshold: call iq_to_bits_batch_auto(captures, p), which detects a threshold per capture",
    "msg_records": "a batch computes no message records: call iq_to_bits(..., msg_records=True) per capture, or a CaptureStream(msg_records=True)",
    "dc_correction": "a batch does not remove the captures' means: call iq_to_bits(..., dc_correction=True) per capture, or a CaptureStream(dc_correction=True)",
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
        raise ValueError(f"a batch demodulates ASK and FSK, not {p.modulation_type}: call iq_to_bits per capture, or push the captures "
                         "through a CaptureStream (a Costas loop in one wavefront lane is not worth having)")


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

    def __init__(self, items, params, lengths, qads=None, rerun=None, noise=None, noise_flags=None):
        self._items = list(items)
        self.params = params
        self.lengths = [int(n) for n in lengths]
        self._qads = qads                  # per capture: device tensor or None
        self._rerun = rerun                # k, cap_rows -> (HostBits, qad)
        # iq_to_bits_batch_auto: detect_noise_level's value per capture (Python floats) and urhgpu_noise_result's flag per capture -- 1 the
        # capture was gated with its value; 2 the value is not below the sample type's max_magnitude: the reference slices zeros(2), and so
        # did the batch (n_samples = 2); 0 the reference raises, and so does handing that capture out (the value is the NaN / infinity)
        self.noise = None if noise is None else [float(x) for x in noise]
        self.noise_flags = None if noise_flags is None else [int(f) for f in noise_flags]

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

    def retry(self, k):
        """a truncated capture once more, alone, with the row capacity its first run reported; the result takes its place"""
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


def _run_batch(pipe, caps, lengths, npdt, p, want_qad, cap_rows, pool, device_iq=None, device_starts=None, auto_noise=False):
    """the short captures of a batch through the three launches.  caps: numpy arrays (packed and uploaded here, one copy), or device_iq (a
    device tensor that holds them back to back) with device_starts.  auto_noise: four launches -- every capture gated with the threshold
    detected for it (urhgpu_iq_to_bits_batch_auto_dev) -- and one more read, of the K result blocks; "only": that first launch and that
    read alone.  Returns (HostBits list, qad tensor or None, device input, starts, (noise values, flags) or None)."""
    torch, lib = pipe.torch, _lib.load()
    k = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    cp = p.to_c(npdt)
    cp.write_bit_sample_pos = 0
    plan, work_bytes, blob_cap = batch_plan(lengths, cp, cap_rows)
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
        _lib.check(lib.urhgpu_batch_noise_dev(pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), C.c_void_p(d_plan), k, C.byref(cp),
                                              C.c_void_p(d_noise.data_ptr())))
        return None, None, (dev_in, meta_bytes, device_iq), starts, fetch_noise()
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device) if want_qad else None
    work = pipe._buf("batch:work", (max(work_bytes, 16),), torch.uint8)
    counts = pipe._buf("batch:counts", (8 * max(k, 1),), torch.int64)
    d_dir = pipe._buf("batch:dir", (k + 1,), torch.int64)
    blob = pipe._buf("batch:blob", (max(blob_cap, 16),), torch.uint8)
    args = (pipe.ctx.handle, C.c_void_p(d_iq), total, C.c_void_p(d_start), C.c_void_p(d_plan), k, C.byref(cp),
            C.c_void_p(qad.data_ptr()) if qad is not None else None, C.c_void_p(work.data_ptr()), work_bytes,
            C.c_void_p(counts.data_ptr()), C.c_void_p(d_dir.data_ptr()), C.c_void_p(blob.data_ptr()), blob_cap)
    if auto_noise:
        _lib.check(lib.urhgpu_iq_to_bits_batch_auto_dev(*args, C.c_void_p(d_noise.data_ptr())))
    else:
        _lib.check(lib.urhgpu_iq_to_bits_batch_dev(*args))
    h_dir = _pinned(torch, pool, "batch_dir", 8 * (k + 1))
    h_blob = _pinned(torch, pool, "batch_blob", min(blob_cap, FIRST_BLOB_BUFFER_BYTES))
    got = C.c_int64(0)

    def fetch():
        return lib.urhgpu_batch_fetch(pipe.ctx.handle, C.c_void_p(d_dir.data_ptr()), k, C.c_void_p(blob.data_ptr()), C.c_void_p(h_dir.data_ptr()),
                                      C.c_void_p(h_blob.data_ptr()), int(h_blob.numel()), C.byref(got))
    st = fetch()
    if st == _lib.ERR_CAPACITY and int(got.value) > h_blob.numel():
        h_blob = _pinned(torch, pool, "batch_blob", int(got.value))             # larger than the buffer so far: grow to what it needs, fetch again
        st = fetch()
    _lib.check(st)
    if int(got.value) > blob_cap:
        raise _lib.UrhGpuError(_lib.ERR_CAPACITY, "the batch's blobs did not fit the planned capacity")
    noise = fetch_noise() if auto_noise else None
    offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
    items = []
    for i in range(k):
        n_i = 2 if (noise is not None and noise[1][i] == 2) else int(lengths[i])      # flag 2: the reference slices zeros(2), and so did the device
        h = HostBits.from_blob(h_blob.data_ptr() + int(offs[i]), p, seq=i, n_samples=n_i,
                               d_qad=(qad.data_ptr() + 4 * int(starts[i])) if qad is not None else 0)
        h._keep = (h_blob, qad)
        items.append(h)
    return items, qad, (dev_in, meta_bytes, device_iq), starts, noise


def iq_to_bits_batch(pipe, captures, p, want_qad=False, cap_rows=None, long_from=None, _pool=None, **options):
    """DevicePipeline.iq_to_bits_batch (see there)"""
    check_batch_options(p, **options)
    return _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, False)


_NOT_IN_A_BATCH_AUTO = {
    "auto_center": "a batch slices every capture with p.center: call iq_to_bits(..., auto_noise=True, auto_center=True) per capture, or a CaptureStream",
    "msg_records": "a batch computes no message records: call iq_to_bits(..., auto_noise=True, msg_records=True) per capture, or a CaptureStream",
    "dc_correction": "a batch does not remove the captures' means: call iq_to_bits(..., auto_noise=True, dc_correction=True) per capture, or a CaptureStream",
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


def _batch(pipe, captures, p, want_qad, cap_rows, long_from, _pool, auto_noise):
    """iq_to_bits_batch and iq_to_bits_batch_auto: the input forms, the routing by length, the result sequence"""
    torch = pipe.torch
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    pool = pipe._pinned if _pool is None else _pool
    from .pipeline import _torch_dtype
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
    short, long_ = route(lengths, long_from)
    items = [None] * len(caps)
    qads = [None] * len(caps) if want_qad else None
    noise, flags = ([0.0] * len(caps), [1] * len(caps)) if auto_noise else (None, None)

    # the short ones: one batch
    sub = [caps[i] for i in short]
    sub_len = [lengths[i] for i in short]
    if on_device:
        if packed and len(long_) == 0 and cat.is_contiguous():
            dev_cat, dev_starts = cat, starts_in
        else:
            dev_cat = torch.cat(sub) if sub else torch.empty((0, 2), dtype=caps[0].dtype if caps else torch.float32, device=pipe.device)
            dev_starts = None
        dev_cat = dev_cat.contiguous()
        got, qad, src, starts, found = _run_batch(pipe, None, sub_len, npdt, p, want_qad, cap_rows, pool, device_iq=dev_cat, device_starts=dev_starts,
                                                  auto_noise=auto_noise)
    else:
        got, qad, src, starts, found = _run_batch(pipe, sub, sub_len, npdt, p, want_qad, cap_rows, pool, auto_noise=auto_noise)
    if auto_noise == "only":
        return found
    for j, i in enumerate(short):
        items[i] = got[j]
        items[i].seq = int(i)
        if auto_noise:
            noise[i], flags[i] = found[0][j], found[1][j]
        if want_qad:
            qads[i] = qad[int(starts[j]):int(starts[j]) + items[i].n_samples]     # (an auto_noise capture that is gated entirely: zeros(2))

    # the long ones: an ordinary pass each
    p_pass = replace(p, write_bit_sample_pos=False)
    for i in long_:
        c = caps[i]
        t = c if on_device else torch.from_numpy(c).to(pipe.device)
        res = pipe.iq_to_bits(t.contiguous(), p_pass, want_qad=want_qad, cap_rows=cap_rows if isinstance(cap_rows, int) else None,
                              auto_noise=bool(auto_noise))
        if auto_noise:
            flags[i] = res.noise_flag
            noise[i] = float(res._noise)
            if flags[i] == 0:                              # the reference raises for this capture: nothing to hand out
                continue
        h = res.host(pool={})
        h.seq = int(i)
        items[i] = h
        if want_qad:
            qads[i] = res.qad.clone()

    def rerun(k, rows):
        """capture k alone with `rows` rows of capacity, results in pinned memory of their own"""
        c = caps[k]
        t = c if on_device else torch.from_numpy(c).to(pipe.device)
        if auto_noise:                                     # (alone through the same entry point: it detects the same threshold)
            one = iq_to_bits_batch_auto(pipe, [t.contiguous()], p, want_qad=want_qad, cap_rows=int(rows), long_from=long_from, _pool={})
        else:
            one = iq_to_bits_batch(pipe, [t.contiguous()], p, want_qad=want_qad, cap_rows=int(rows), long_from=long_from, _pool={})
        return one[0], (one.qad(0) if want_qad else None)

    return BatchBits(items, p, lengths, qads, rerun, noise, flags)


def launch_counts(pipe):
    """(kernel launches, copies) the batch entry points have issued on the pipeline's context so far: 3 and 2 per batch, 4 and 3 per batch
    with automatic noise thresholds, 1 and 1 per detect_noise_levels"""
    out = (C.c_int64 * 2)()
    _lib.check(_lib.load().urhgpu_batch_launches(pipe.ctx.handle, out))
    return int(out[0]), int(out[1])
