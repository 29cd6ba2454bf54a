"""Live sniffing on the GPU: the counterpart of ProtocolSniffer.__demodulate_data
(src/urh/signalprocessing/ProtocolSniffer.py:204-281 of the reference), the reference's live mode and the CLI's RX mode.

The sniffer receives a few milliseconds of samples at a time.  Per chunk it decides whether the chunk is signal or noise
(RMS per component against the noise threshold), optionally adapts the threshold, and accumulates chunks until a
transmission has ended (10 symbols of noise, or a full buffer); only then the accumulated samples are demodulated,
optionally after the center has been detected again.

Two layers:

  LiveSniffer      the state machine of the reference, written with the reference's own scalar expressions (so that the noise
                   threshold carries the reference's scalar type: a Python float until the first adaptive update, then
                   numpy.float32 for float32 chunks / numpy.float64 for integer chunks).  It holds no samples.
  engine           where the samples live and where the O(n) work happens:
                       stats_append(chunk, index) -> (sum, max)   sum and maximum of chunk ** 2.0 over the 2n components in the
                                                                  reference's arithmetic, the chunk stored at row `index` of the
                                                                  accumulation buffer (trimmed as the reference trims it)
                       flush(index, params, automatic_center) -> (center, bits, pauses, bit_sample_pos)
                   GpuSniffEngine is the product: the buffer is device resident, a chunk costs one pass of
                   urhgpu_chunk_power_stats_dev (append + statistics in one read, two launches, one synchronisation), a flush is
                   DevicePipeline.iq_to_bits on buffer[:index] (with automatic_center: auto_center=True, the center detected inside the pass).  There is no CPU engine in this package.
"""
import time
from dataclasses import dataclass, replace

import numpy as np

from . import _lib
from .signal_functions import dtype_code

DEFAULT_BUFFER_SAMPLES = int(100 * 1000 * 1000 / 8)      # ProtocolSniffer.BUFFER_SIZE_MB = 100 (:30, :116-118): rows, whatever the dtype
SNIFF_PAUSE_THRESHOLD = 8                                # _ppseq_to_bits' default: the sniffer does not pass the signal's (:263-268)


def trimmed_rows(n: int, index: int, buffer_len: int) -> int:
    """rows of an n-row chunk that __add_to_buffer stores at `index` (:97-106): a chunk that does not fit loses one row more than it must"""
    if n + index > buffer_len:
        n = buffer_len - index - 1
    return n


def max_magnitude(dtype) -> float:
    """Signal.max_magnitude (Signal.py:404-406): from it on the reference does not demodulate (quad_demod, :474-484)"""
    dtype = np.dtype(dtype)
    mi, ma = (-1, 1) if dtype.kind == "f" else (int(np.iinfo(dtype).min), int(np.iinfo(dtype).max))
    return (2 * max(mi ** 2, ma ** 2)) ** 0.5


@dataclass
class SniffedMessage:
    """What the sniffer hands to urh's Message constructor (:270-281): no RSSI, no padding to a message length divisor."""
    plain_bits: object               # array('B')
    pause: int
    first_bit_sample_pos: int        # bit_sample_pos[i][0], in samples from the start of the flushed buffer
    timestamp: float
    samples_per_symbol: int
    bits_per_symbol: int

    @property
    def plain_bits_str(self):
        return "".join(map(str, self.plain_bits))


class GpuSniffEngine:
    """Device-resident accumulation buffer + the per-chunk pass + the flush, on a DevicePipeline."""

    def __init__(self, pipe, dtype=np.float32, buffer_samples=DEFAULT_BUFFER_SAMPLES, apply_dc_correction=False):
        import torch
        self.apply_dc_correction = bool(apply_dc_correction)   # every chunk minus its own mean before anything else sees it (Device.py:822-823)
        self.torch = torch
        self.pipe = pipe
        self.dtype = np.dtype(dtype)
        self.code = dtype_code(self.dtype)
        self.tdtype = {np.dtype(np.int8): torch.int8, np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16,
                       np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32}[self.dtype]
        self.buffer_len = int(buffer_samples)
        self.buffer = torch.empty((self.buffer_len, 2), dtype=self.tdtype, device=pipe.device)
        self._spill = None               # device copy of a host chunk that is trimmed (statistics span the whole chunk)
        self._sum, self._max = _lib.C.c_double(0.0), _lib.C.c_double(0.0)

    def stats_append(self, chunk, index: int):
        """chunk: (n, 2) numpy array (uploaded straight to its rows of the buffer) or device tensor (copied by the statistics pass)."""
        torch = self.torch
        n = int(chunk.shape[0])
        store = max(trimmed_rows(n, index, self.buffer_len), 0)
        dst = self.buffer[index:index + store]
        if self.apply_dc_correction:
            chunk = self._dc_corrected(chunk)                  # a device tensor of the engine's: the caller's chunk is left as it is
        if isinstance(chunk, np.ndarray):
            if chunk.dtype != self.dtype or chunk.ndim != 2 or chunk.shape[1] != 2:
                raise ValueError(f"chunk must be an (n, 2) array of {self.dtype}")
            # straight from the receive process's array: the runtime moves pageable memory through its own pinned staging area, which
            # measured faster than a staging tensor of ours (one host copy less; tools/sniffer_probe.py)
            staged = torch.from_numpy(np.ascontiguousarray(chunk))
            if store == n:
                dst.copy_(staged, non_blocking=True)
                src, dst_ptr, store = dst, None, 0                              # statistics over the rows where they landed, nothing to store
            else:
                if self._spill is None or self._spill.shape[0] < n:
                    self._spill = torch.empty((n, 2), dtype=self.tdtype, device=self.pipe.device)
                src = self._spill[:n]
                src.copy_(staged, non_blocking=True)
                dst_ptr = dst.data_ptr()
        else:
            if chunk.dtype != self.tdtype or chunk.dim() != 2 or chunk.shape[1] != 2 or not chunk.is_contiguous() or chunk.device != self.buffer.device:
                raise ValueError(f"chunk must be a contiguous (n, 2) tensor of {self.tdtype} on {self.buffer.device}")
            src, dst_ptr = chunk, dst.data_ptr()
        ctx = self.pipe.ctx
        ctx.set_stream(torch.cuda.current_stream(self.pipe.device).cuda_stream)
        _lib.check(_lib.load().urhgpu_chunk_power_stats_dev(ctx.handle, _lib.C.c_void_p(src.data_ptr()), self.code, n, _lib.C.c_void_p(dst_ptr), store,
                                                            _lib.C.byref(self._sum), _lib.C.byref(self._max)))
        if self.dtype == np.float32:
            return np.float32(self._sum.value), np.float32(self._max.value)     # float32 values, widened exactly by the library
        return np.float64(self._sum.value), np.float64(self._max.value)

    def _dc_corrected(self, chunk):
        """the chunk minus its mean (urhgpu_dc_correct_dev, queued in front of the statistics pass), in the engine's spill rows"""
        from .filter import dc_correct_dev
        torch = self.torch
        n = int(chunk.shape[0])
        if self._spill is None or self._spill.shape[0] < n:
            self._spill = torch.empty((n, 2), dtype=self.tdtype, device=self.pipe.device)
        rows = self._spill[:n]
        if isinstance(chunk, np.ndarray):
            if chunk.dtype != self.dtype or chunk.ndim != 2 or chunk.shape[1] != 2:
                raise ValueError(f"chunk must be an (n, 2) array of {self.dtype}")
            rows.copy_(torch.from_numpy(np.ascontiguousarray(chunk)), non_blocking=True)
            return dc_correct_dev(self.pipe, rows, out=rows)
        if chunk.dtype != self.tdtype or chunk.dim() != 2 or chunk.shape[1] != 2 or not chunk.is_contiguous() or chunk.device != self.buffer.device:
            raise ValueError(f"chunk must be a contiguous (n, 2) tensor of {self.tdtype} on {self.buffer.device}")
        return dc_correct_dev(self.pipe, chunk, out=rows)

    def launches(self) -> int:
        """kernel launches the per-chunk pass has issued so far (two per chunk, whatever its length)"""
        out = _lib.C.c_int64(0)
        _lib.check(_lib.load().urhgpu_chunk_stats_launches(self.pipe.ctx.handle, _lib.C.byref(out)))
        return int(out.value)

    def flush(self, index: int, params, automatic_center: bool):
        from . import estimators
        torch, pipe = self.torch, self.pipe
        iq = self.buffer[:index]
        sps = int(params.samples_per_symbol)
        center = params.center
        if not (params.noise_threshold < max_magnitude(self.dtype)):           # Signal.quad_demod (:474-484): two zeros instead of a demodulation
            qad = torch.zeros(2, dtype=torch.float32, device=pipe.device)
        elif automatic_center:
            # ProtocolSniffer.py:246-249: detect_center(qad, max_size=150 * samples_per_symbol) per flush -- ONE queued pass that demodulates,
            # finds the center on the device and slices with it (the exact row bound: no second pass for a noisy buffer)
            res = pipe.iq_to_bits(iq, params, want_qad=True, cap_rows=index // (int(params.tolerance) + 1) + 2, auto_center=True,
                                  center_max_size=150 * sps)
            center = res.center
            if center is None:
                raise ValueError("no center could be detected (the reference fails in grab_pulse_lens with center None)")
            res.check_capacity()
            return (center,) + tuple(res.messages())
        else:
            res = pipe.iq_to_bits_checked(iq, params, want_qad=False)
            return (center,) + tuple(res.messages())
        if automatic_center:
            center = estimators.detect_center_dev(pipe, qad, max_size=150 * sps)
            if center is None:
                raise ValueError("no center could be detected (the reference fails in grab_pulse_lens with center None)")
        res = pipe.qad_to_bits(qad, replace(params, center=center))
        res.check_capacity()
        return (center,) + tuple(res.messages())


class LiveSniffer:
    """feed(chunk) is ProtocolSniffer.__demodulate_data(data): it returns the messages that chunk completed (usually none)."""

    def __init__(self, pipe, params, dtype=np.float32, sample_rate=1e6, adaptive_noise=False, automatic_center=False,
                 buffer_samples=DEFAULT_BUFFER_SAMPLES, clock=time.time, engine=None, trace=False, apply_dc_correction=False):
        """apply_dc_correction: every fed chunk minus its own mean, on the device, before it is appended and its gate statistics are taken
        -- the reference's receive path in front of the sniffer (Device.py:822-823, on by default there).  Off: the chunks as they are fed."""
        self.params = params
        self.dtype = np.dtype(dtype)
        self.sample_rate = sample_rate
        self.adaptive_noise = adaptive_noise
        self.automatic_center = automatic_center
        self.clock = clock
        if engine is not None and apply_dc_correction and not getattr(engine, "apply_dc_correction", False):
            raise ValueError("apply_dc_correction with an engine of the caller's: the engine must correct its chunks itself")
        self.engine = engine if engine is not None else GpuSniffEngine(pipe, self.dtype, buffer_samples, apply_dc_correction)
        self.buffer_len = int(buffer_samples)
        self.noise_threshold = params.noise_threshold       # a Python float until the first adaptive update (see feed)
        self.center = params.center
        self.pause_length = 0
        self.index = 0                                      # __current_buffer_index
        self.messages = []
        self.centers = []                                   # the center of every flush
        self.trace = [] if trace else None

    def clear(self):
        """ProtocolSniffer.clear (:292-294)"""
        self.index = 0
        self.messages.clear()

    def _buffer_is_full(self):
        return self.index >= self.buffer_len - 2            # :111-112

    def _add_to_buffer(self, n):
        self.index += trimmed_rows(n, self.index, self.buffer_len)

    def feed(self, chunk):
        n = int(chunk.shape[0])
        if n == 0:                                          # :210-211 (nothing happens, nothing is traced as a decision)
            return self._traced(None, False, [])
        # the engine stores the chunk at `index` in the same pass that reads it for the statistics: rows beyond the committed index are
        # harmless when the decision below is not to append
        total, peak = self.engine.stats_append(chunk, self.index)
        with np.errstate(all="ignore"):
            # np.sqrt(np.mean(power_spectrum)): np.mean is the sum divided by the 2n components in the chunk's float type
            mean = total / total.dtype.type(2 * n)
            is_above_noise = bool(np.sqrt(mean) > self.noise_threshold)
            if self.adaptive_noise and not is_above_noise:
                value = 0.9 * self.noise_threshold + 0.1 * np.sqrt(peak)       # :216-220, written as the reference writes it
                if value != self.noise_threshold:                              # Signal.noise_threshold's setter (Signal.py:388-393)
                    self.noise_threshold = value
        if is_above_noise:
            self._add_to_buffer(n)
            self.pause_length = 0
            if not self._buffer_is_full():
                return self._traced(is_above_noise, False, [])
        else:
            self.pause_length += n
            if self.pause_length < 10 * self.params.samples_per_symbol:
                self._add_to_buffer(n)
                if not self._buffer_is_full():
                    return self._traced(is_above_noise, False, [])
        if self.index == 0:
            return self._traced(is_above_noise, False, [])
        return self._traced(is_above_noise, True, self._flush())

    def _flush(self):
        index = self.index
        timestamp = self.clock() - (index / self.sample_rate)                  # of the first sample in the buffer (:240-242)
        self.index = 0
        p = replace(self.params, noise_threshold=self.noise_threshold, center=self.center, pause_threshold=SNIFF_PAUSE_THRESHOLD,
                    write_bit_sample_pos=True)
        center, bit_data, pauses, bit_sample_pos = self.engine.flush(index, p, self.automatic_center)
        self.center = center
        self.centers.append(center)
        sps = self.params.samples_per_symbol
        new = []
        for i, (bits, pause) in enumerate(zip(bit_data, pauses)):
            first = bit_sample_pos[i][0]
            new.append(SniffedMessage(bits, int(pause), int(first), timestamp + (first / self.sample_rate), sps, int(self.params.bits_per_symbol)))
        self.messages.extend(new)
        return new

    def _traced(self, above, flushed, new):
        if self.trace is not None:
            self.trace.append({"above": above, "noise": self.noise_threshold, "pause_length": self.pause_length, "index": self.index,
                               "flushed": flushed, "n_messages": len(self.messages)})
        return new
