"""A batch in which every capture has its OWN parameters (include/urhgpu.h "a batch of captures: parameters per capture";
urh_amd/csrc/batch_each.hip): the per-capture table and its thresholds, the plan made of it, the one upload, the launches, the results."""
import ctypes as C
from dataclasses import replace

import numpy as np

from .. import _lib
from ..host_bits import HostBits
from ..signal_functions import dtype_code, mod_code
from .inputs import LONG_FROM_DEFAULT, _batch_input, back_to_back, route
from .options import check_batch_each_options
from .run import BatchBits
from .staging import _pinned, captures_at, noise_buffer, read_noise_blocks, upload, write_noise_blocks
from .walk import _fetch_blobs, _fetch_records, record_capacity, walk_buffers

EACH_DTYPE = np.dtype([("mod", "<i4"), ("bits_per_symbol", "<i4"), ("samples_per_symbol", "<u4"), ("tolerance", "<i4"), ("pause_threshold", "<i8"),
                       ("noise_val", "<f4"), ("thr_first", "<i4")])     # struct urhgpu_batch_each (_lib.BatchEach)
assert EACH_DTYPE.itemsize == C.sizeof(_lib.BatchEach) == 32


def each_table(params, npdt=np.float32):
    """(urhgpu_batch_each[K] as a numpy record array, float32[sum(order_k - 1)] thresholds): capture k's record from params[k] and its slicing
    thresholds from urhgpu_get_center_thresholds, the function a pass over one capture uses.  The ranges are DemodParams.to_c's: what the
    reference itself fails on raises the same exception.  Host arithmetic: works without a GPU."""
    lib = _lib.load()
    table = np.zeros(len(params), EACH_DTYPE)
    n_thr = sum((1 << int(p.bits_per_symbol)) - 1 for p in params if 1 <= int(p.bits_per_symbol) <= 7)
    thr = np.zeros(n_thr, np.float32)
    at = 0
    for e, p in zip(table, params):
        cp = p.to_c(npdt)
        if cp.bits_per_symbol > 7:
            raise _lib.UrhGpuError(_lib.ERR_UNSUPPORTED, "bits_per_symbol above 7")
        order = 1 << cp.bits_per_symbol
        _lib.check(lib.urhgpu_get_center_thresholds(cp.center, cp.center_spacing, order, thr[at:].ctypes.data_as(C.POINTER(C.c_float))))
        e["mod"], e["bits_per_symbol"], e["samples_per_symbol"], e["tolerance"] = cp.mod, cp.bits_per_symbol, cp.samples_per_symbol, cp.tolerance
        e["pause_threshold"], e["noise_val"], e["thr_first"] = cp.pause_threshold, 0.0 if cp.mod == _lib.MOD_ASK else -4.0, at
        at += order - 1
    return table, thr


def batch_plan_each(lengths, table, cap_rows=None):
    """urhgpu_batch_plan_each: batch_plan with every capture's own tolerance, samples per symbol and bits per symbol (its record of `table`);
    the launch order holds the ASK captures first, then the FSK captures, each group longest first.  Host arithmetic: works without a GPU."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    table = np.ascontiguousarray(table, dtype=EACH_DTYPE)
    k = int(lengths.size)
    if len(table) != k:
        raise ValueError("the table holds one record per capture")
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
    _lib.check(_lib.load().urhgpu_batch_plan_each(lengths.ctypes.data_as(C.c_void_p), k, table.ctypes.data_as(C.c_void_p), policy, fixed,
                                                  plan.ctypes.data_as(C.c_void_p), C.byref(work), C.byref(blob)))
    return plan, int(work.value), int(blob.value)


def _run_each(pipe, pool, caps, lengths, npdt, params, auto_noise, divisor, want_qad, cap_rows, device_iq=None, device_starts=None, noise_flags=None):
    """the short captures through ONE batch: THE upload (starts, plan, the table, the noise blocks, the thresholds -- and host captures'
    samples -- in one copy), the launches, the fetches.  Returns (HostBits list, qad buffer or None, starts, (noise values, flags) or None)."""
    torch, lib = pipe.torch, _lib.load()
    k = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    table, thr = each_table(params, npdt)
    plan, work_bytes, blob_cap = batch_plan_each(lengths, table, cap_rows)
    starts = back_to_back(lengths) if device_starts is None else np.asarray(device_starts, dtype=np.int64)
    total = int(starts[-1]) if device_iq is None else int(device_iq.shape[0])
    item = 2 * np.dtype(npdt).itemsize
    # the tables behind starts and plan: one int64 of padding (the records are 16-byte aligned), the K records, the K noise blocks, the thresholds
    blocks = np.zeros(8 * k, np.int64)
    if not auto_noise and k:
        write_noise_blocks(blocks.ctypes.data, [p.noise_threshold for p in params])
        if noise_flags is not None:                        # (a threshold that is not below the sample type's max_magnitude: two zeros are walked)
            for r, flag in zip((_lib.NoiseResult * k).from_address(blocks.ctypes.data), noise_flags):
                r.flag = int(flag)
    thr64 = np.zeros((len(thr) + 1) // 2, np.int64)
    thr64.view(np.float32)[:len(thr)] = thr
    up = upload(pipe, lambda n: _pinned(torch, pool, "batch_stage", n), lambda n: torch.empty(n, dtype=torch.uint8, device=pipe.device), starts, plan,
                tables=(np.zeros(1, np.int64), table.view(np.int64), blocks, thr64), payload_bytes=total * item if device_iq is None else 0,
                fill=captures_at(caps, starts, item) if device_iq is None else None)
    d_iq = up.d_payload if device_iq is None else device_iq.data_ptr()
    d_each = up.d_tables + 8
    d_blocks = d_each + 32 * k
    d_thr = d_blocks + 64 * k
    d_noise = noise_buffer(pipe, k) if auto_noise else None
    qad = torch.empty(max(total, 1), dtype=torch.float32, device=pipe.device) if want_qad else None
    bufs = walk_buffers(pipe, k, work_bytes, blob_cap)
    n_ask = int((table["mod"] == _lib.MOD_ASK).sum())
    dt = dtype_code(npdt)
    _lib.check(lib.urhgpu_iq_to_bits_batch_each_dev(
        pipe.ctx.handle, C.c_void_p(d_iq), total, dt, C.c_void_p(up.d_start), C.c_void_p(up.d_plan), k, C.c_void_p(d_each), C.c_void_p(d_thr), len(thr),
        n_ask, int(bool(auto_noise)), C.c_void_p(qad.data_ptr()) if qad is not None else None, C.c_void_p(bufs.work.data_ptr()), work_bytes,
        C.c_void_p(bufs.counts.data_ptr()), C.c_void_p(bufs.d_dir.data_ptr()), C.c_void_p(bufs.blob.data_ptr()), blob_cap,
        C.c_void_p(d_noise.data_ptr() if auto_noise else d_blocks)))
    queued = None
    if divisor is not None:                                # the records of all captures behind the walk, before anything reuses the work buffer
        cap_rec = record_capacity(plan)
        d_rec = pipe._buf("batch:rec", (C.sizeof(_lib.MsgRecord) * max(cap_rec, 1),), torch.uint8)
        d_cap = pipe._buf("batch:rec_capture", (max(cap_rec, 1),), torch.int32)
        d_rdir = pipe._buf("batch:rec_dir", (k + 1,), torch.int64)
        _lib.check(lib.urhgpu_batch_msg_records_each_dev(
            pipe.ctx.handle, C.c_void_p(d_iq), total, dt, C.c_void_p(up.d_start), C.c_void_p(up.d_plan), k, C.c_void_p(d_each), int(divisor),
            C.c_void_p(bufs.work.data_ptr()), work_bytes, C.c_void_p(bufs.counts.data_ptr()), C.c_void_p(d_rdir.data_ptr()), C.c_void_p(d_rec.data_ptr()),
            cap_rec, C.c_void_p(d_cap.data_ptr())))
        queued = (d_rec, cap_rec)
    h_dir, h_blob = _fetch_blobs(pipe, pool, bufs.d_dir, k, bufs.blob, bufs.blob_cap)
    noise = read_noise_blocks(pipe, pool, d_noise, k) if auto_noise else None
    flags = noise[1] if noise is not None else noise_flags
    offs = h_dir.numpy()[:8 * (k + 1)].view(np.int64)
    items = []
    for j in range(k):
        two = flags is not None and flags[j] == 2          # (the reference slices zeros(2), and so did the device)
        h = HostBits.from_blob(h_blob.data_ptr() + int(offs[j]), params[j], seq=j, n_samples=2 if two else int(lengths[j]),
                               d_qad=(qad.data_ptr() + 4 * int(starts[j])) if qad is not None else 0)
        h._keep = (h_blob, qad, up.dev_in)
        items.append(h)
    if queued is not None:
        _fetch_records(pipe, pool, queued, items)
    return items, qad, starts, noise


def iq_to_bits_batch_each(pipe, captures, params, auto_noise=False, message_length_divisor=None, want_qad=False, cap_rows=None, long_from=None,
                          _pool=None, _noise_flags=None, **options):
    """DevicePipeline.iq_to_bits_batch_each (see there)"""
    given = _batch_input(pipe, captures)
    n = len(given.caps)
    params = check_batch_each_options(params, n, message_length_divisor, **options)
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    pool = pipe._pinned if _pool is None else _pool
    caps, lengths = given.caps, given.lengths
    short, long_ = route(lengths, long_from)
    items = [None] * n
    qads = [None] * n if want_qad else None
    noise, flags = ([0.0] * n, [1] * n) if auto_noise else (None, None)

    dev_cat = dev_starts = None
    if given.on_device:
        dev_cat, dev_starts = given.device_cat(pipe, short)
    got, qad, starts, found = _run_each(pipe, pool, None if dev_cat is not None else [caps[i] for i in short], [lengths[i] for i in short], given.npdt,
                                        [params[i] for i in short], auto_noise, message_length_divisor, want_qad, cap_rows, dev_cat, dev_starts,
                                        None if _noise_flags is None else [_noise_flags[i] for i in short])
    for j, i in enumerate(short):
        items[i] = got[j]
        items[i].seq = int(i)
        if found is not None:
            noise[i], flags[i] = found[0][j], found[1][j]
        if want_qad:
            qads[i] = qad[int(starts[j]):int(starts[j]) + items[i].n_samples]

    # the long ones: an ordinary pass each, with their own parameters
    for i in long_:
        if _noise_flags is not None and _noise_flags[i] == 2:
            raise ValueError(f"capture {i} has {lengths[i]} samples and a noise threshold that gates all of it: a pass has no configured two-zeros "
                             "form (Signal.get_protocol slices it alone)")
        res = pipe.iq_to_bits(given.tensor(pipe, i), replace(params[i], write_bit_sample_pos=False), want_qad=want_qad,
                              cap_rows=cap_rows if isinstance(cap_rows, int) else None, auto_noise=auto_noise,
                              msg_records=message_length_divisor is not None, message_length_divisor=message_length_divisor or 1)
        if auto_noise:
            flags[i] = res.noise_flag
            noise[i] = float(res._noise)
            if flags[i] == 0:                              # the reference raises for this capture: nothing to hand out
                continue
        h = res.host(pool={})
        h.seq = int(i)
        if message_length_divisor is not None:             # a copy of the pass's records: its pinned block belongs to the slot
            from ..protocol import RECORD_DTYPE
            try:
                h.records = res.records.copy()
            except _lib.UrhGpuError:                       # (a capacity was exceeded: message_data() says so, retry(k) repeats the capture)
                h.records = np.zeros(0, RECORD_DTYPE)
        items[i] = h
        if want_qad:
            qads[i] = res.qad.clone()

    def rerun(k, rows):
        """capture k alone with params[k], `rows` rows of capacity and the options of the batch, results in pinned memory of their own"""
        one = iq_to_bits_batch_each(pipe, [given.tensor(pipe, k)], [params[k]], auto_noise, message_length_divisor, want_qad, int(rows), long_from, {},
                                    None if _noise_flags is None else [_noise_flags[k]])
        return one[0], (one.qad(0) if want_qad else None)

    return BatchBits(items, list(params), lengths, qads, rerun, noise, flags)


def params_from_estimates(estimates, base):
    """entry k of DevicePipeline.estimate_batch's result as the DemodParams of capture k, the way Signal._apply_estimate applies it with
    detect_modulation and detect_noise BOTH set: "OOK" becomes ASK with one bit per symbol, bit_length becomes samples_per_symbol, center,
    tolerance, noise and modulation are all taken over (an estimate made with a given noise or modulation returns that one, so taking it
    changes nothing; a caller who wants to keep base's value whatever the estimate says replaces it afterwards); an entry that is None (the
    estimate found no message) keeps `base`.  base: one DemodParams for all, or one per capture.  Host arithmetic."""
    entries = list(estimates)
    bases = [base] * len(entries) if not isinstance(base, (list, tuple)) else list(base)
    if len(bases) != len(entries):
        raise ValueError(f"base holds one DemodParams per capture ({len(entries)}), or is one for all")
    out = []
    for est, p in zip(entries, bases):
        if est is None:
            out.append(p)
            continue
        mod = est["modulation_type"]
        q = replace(p, modulation_type="ASK" if mod == "OOK" else mod, samples_per_symbol=int(est["bit_length"]), center=float(est["center"]),
                    tolerance=int(est["tolerance"]), noise_threshold=float(est["noise"]))
        if mod == "OOK":
            q = replace(q, bits_per_symbol=1)
        out.append(q)
    return out
