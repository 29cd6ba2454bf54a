"""The estimate of a session: every capture's parameters (include/urhgpu.h "a batch of captures: message ranges per capture")."""
import ctypes as C

import numpy as np

from .. import _lib
from .inputs import LONG_FROM_DEFAULT, _batch_input, back_to_back, per_capture, route
from .run import CaptureSequence
from .staging import _pinned, batch_plan, captures_at, detect_noise, order_params, upload, write_noise_blocks

# messages whose centers and plateau decisions go through one native call: urhgpu_msg_estimate refuses (URHGPU_ERR_UNSUPPORTED) more than
# 64 MiB of histogram pool, 4096 counters of 4 bytes per message
MSG_GROUP = 4096

_ESTIMATE_MODULATIONS = ("OOK", "ASK", "FSK", "PSK")
# estimators.estimate_dev agrees with the reference on these sample types (tests/test_gpu_parity.py; tests/test_estimate_routes_gpu.py for the
# unsigned ones, which the reference takes as they stand: magnitudes around the middle of the range, uint16 squares that wrap in C int)
ESTIMATE_SAMPLE_TYPES = (np.float32, np.int8, np.int16, np.uint8, np.uint16)


def check_estimate_options(k, npdt, noise, modulation):
    """(noise per capture, modulation per capture) of estimate_batch, or ValueError with a sentence (host arithmetic: no GPU needed)"""
    if np.dtype(npdt) not in [np.dtype(t) for t in ESTIMATE_SAMPLE_TYPES]:
        raise ValueError(f"estimate_batch takes float32, int8, uint8, int16 and uint16 captures, not {np.dtype(npdt).name}: estimate_dev is not verified "
                         "against the reference on that sample type")

    def check_mod(m):
        if m is not None and m not in _ESTIMATE_MODULATIONS:
            raise ValueError("Unsupported Modulation")           # (what the reference raises, AutoInterpretation.py:394)
    mods = per_capture(modulation, k, "modulation", check_mod)
    noises = [None if v is None else float(v) for v in per_capture(noise, k, "noise")]
    return noises, mods


class BatchEstimates(CaptureSequence):
    """The results of estimate_batch: a sequence with one entry per capture in the order given -- the dict estimators.estimate_dev returns
    (modulation_type, bit_length, center, tolerance, noise), or None.  A capture for which the reference raises (detect_noise_level on a
    capture whose magnitudes hold a NaN or an infinity) raises the same exception where it is handed out, as BatchBits does; the others are
    handed out."""

    def __init__(self, items, errors, lengths):
        self._items, self._errors = list(items), list(errors)
        self.lengths = [int(n) for n in lengths]

    def _hand_out(self, k):
        if self._errors[k] is not None:
            raise self._errors[k]
        return self._items[k]


class _Session:
    """the short captures of a session on the device: the samples back to back, their starts, the plan's launch order and the regions of
    the segmentation, uploaded with ONE copy"""

    def __init__(self, pipe, pool, given, idx=None):
        """the captures idx (None: all) of a batch's input; a packed device tensor that is taken whole is read where it lies"""
        torch = self.torch = pipe.torch
        self.pipe, self.pool, self.npdt = pipe, pool, np.dtype(given.npdt)
        lengths = given.lengths if idx is None else [given.lengths[i] for i in idx]
        caps = None if given.on_device else (given.caps if idx is None else [given.caps[i] for i in idx])
        device_iq, device_starts = given.device_cat(pipe, idx) if given.on_device else (None, None)
        k = self.k = len(lengths)
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.cp = order_params().to_c(self.npdt)                                    # (of the plan only the launch order is read)
        plan, _, _ = batch_plan(self.lengths, self.cp)
        starts = self.starts = back_to_back(self.lengths) if device_starts is None else np.asarray(device_starts, dtype=np.int64)
        self.total = int(starts[-1]) if device_iq is None else int(device_iq.shape[0])
        self.seg_caps = self.lengths // 20 + 1                                      # urhgpu_batch_segments_capacity
        regions = back_to_back(self.seg_caps)
        self.cap_seg = int(regions[-1])
        item = 2 * self.npdt.itemsize
        # THE upload: starts, plan, regions and every sample in one copy
        up = upload(pipe, lambda n: _pinned(torch, pool, "estimate_stage", n), lambda n: pipe._buf("estimate:in", (max(n, 16),), torch.uint8), starts, plan,
                    tables=(regions[:-1],), payload_bytes=self.total * item if device_iq is None else 0,
                    fill=captures_at(caps, starts, item) if device_iq is None else None)
        self.dev_in, self.meta_bytes = up.dev_in, up.meta_bytes
        self.d_start, self.d_plan, self.d_region = up.d_start, up.d_plan, up.d_tables
        if device_iq is None:
            from ..iq_array import _torch_dtype_for
            self.iq = self.dev_in[up.meta_bytes:up.in_bytes].view(_torch_dtype_for(self.npdt)).reshape(self.total, 2)
        else:
            self.iq = device_iq

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
        with np.errstate(all="ignore"):                                             # (a threshold beyond float32, or a NaN, is no news here)
            view[:4 * k].view(np.float32)[:] = np.asarray(noise, dtype=np.float64).astype(np.float32)
            write_noise_blocks(stage.data_ptr() + thr_bytes, noise)
        dev = self.pipe._buf("estimate:noise_in", (nbytes,), torch.uint8)
        dev.copy_(stage[:nbytes], non_blocking=True)
        self.d_thr, self.d_noise_blocks = dev.data_ptr(), dev.data_ptr() + thr_bytes

    def segments(self):
        """urhgpu_batch_segments_dev and its fetch with the thresholds uploaded last: three launches and two copies -> one int64 (n, 2) array
        per capture, relative to the capture's first sample"""
        torch, k, lib, pipe = self.torch, self.k, _lib.load(), self.pipe
        cap = max(self.cap_seg, 1)
        seg = pipe._buf("estimate:seg", (2 * cap,), torch.int64)
        out = pipe._buf("estimate:seg_out", (2 * cap,), torch.int64)
        counts = pipe._buf("estimate:seg_counts", (max(k, 1),), torch.int64)
        d_dir = pipe._buf("estimate:seg_dir", (k + 1,), torch.int64)
        from ..signal_functions import dtype_code
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
        torch, pipe = self.torch, self.pipe
        cp = order_params(mod).to_c(self.npdt)
        qad = pipe._buf("estimate:qad_" + mod, (max(self.total, 1),), torch.float32)
        _lib.check(_lib.load().urhgpu_batch_demod_dev(pipe.ctx.handle, C.c_void_p(self.iq.data_ptr()), self.total, C.c_void_p(self.d_start), C.c_void_p(self.d_plan),
                                                      self.k, C.byref(cp), C.c_void_p(self.d_noise_blocks), C.c_void_p(qad.data_ptr())))
        return qad


def segment_messages_batch(pipe, captures, noise, _pool=None):
    """DevicePipeline.segment_messages_batch (see there)"""
    pool = pipe._pinned if _pool is None else _pool
    given = _batch_input(pipe, captures)
    noises = [float(v) for v in per_capture(noise, len(given.caps), "noise")]
    s = _Session(pipe, pool, given)
    s.upload_noise(noises)
    return s.segments()


def estimate_batch(pipe, captures, noise=None, modulation=None, long_from=None, _pool=None):
    """DevicePipeline.estimate_batch (see there)"""
    from .. import estimators as E
    from ..pipeline import raise_noise_error
    pool = pipe._pinned if _pool is None else _pool
    long_from = LONG_FROM_DEFAULT if long_from is None else int(long_from)
    given = _batch_input(pipe, captures)
    caps, lengths = given.caps, given.lengths
    k_all = len(caps)
    noises, mods = check_estimate_options(k_all, given.npdt, noise, modulation)
    items, errors = [None] * k_all, [None] * k_all

    def alone(i):
        """capture i through estimate_dev: a long capture, or PSK -- the estimate does not pool PSK captures through k_batch_costas"""
        try:
            items[i] = E.estimate_dev(pipe, given.tensor(pipe, i), noise=noises[i], modulation=mods[i])
        except (ValueError, OverflowError) as e:              # what the reference raises for this capture: raised where it is handed out
            errors[i] = e

    by_length, long_ = route(lengths, long_from)
    short = [int(i) for i in by_length if mods[i] != "PSK"]
    for i in sorted([int(i) for i in long_] + [int(i) for i in by_length if mods[i] == "PSK"]):
        alone(i)
    k = len(short)
    if k == 0:
        return BatchEstimates(items, errors, lengths)
    s = _Session(pipe, pool, given, short)

    # 1. noise: detected per capture (one launch, one read), or given
    value = [noises[i] for i in short]
    if any(v is None for v in value):
        found, flags = detect_noise(pipe, pool, s.iq.data_ptr(), s.total, s.d_start, s.d_plan, k, s.cp)
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
