"""Per-rank GPU engine of the sharded IQ->bits pass: the four urhgpu_shard_* phases of liburhgpu.so
(include/urhgpu.h) behind the engine interface urh_amd/sharding/pipeline.py orchestrates.  torch is plumbing
(device buffers, the stream, the tensors the all-gathers move); all arithmetic is in the HIP kernels."""
import ctypes as C

import numpy as np

from . import _lib
from .host_bits import HostBits
from .pipeline import DevicePipeline, PassResult, _torch_dtype


class ShardResult(PassResult):
    """This rank's piece of a sharded result (device tensors) + host views for `sharding.stitch`."""

    _host = None                                            # host results: (engine, blob slot, bytes copied, pass) until looked at, then the HostBits

    def piece(self):
        """dict(rows, bits, msg_end, pauses, pos, pos_end) of numpy arrays (see sharding.stitch)."""
        self.check_capacity()
        n_rows, n_msg, n_bits, n_pos = self.host_counts()
        rows = self.rows_buf[:n_rows].cpu().numpy()
        if n_rows and rows[0, 0] == _lib.ROW_ABSORBED:
            rows = rows[1:]
        return dict(rows=rows, bits=self.bits_buf[:n_bits].cpu().numpy(),
                    msg_end=self.msg_off_buf[1:n_msg + 1].cpu().numpy(), pauses=self.pauses_buf[:n_msg].cpu().numpy(),
                    pos=self.pos_buf[:n_pos].cpu().numpy() if self.pos_buf is not None else np.zeros(0, np.int64),
                    pos_end=self.pos_off_buf[1:n_msg + 1].cpu().numpy())

    def host(self):
        """This rank's piece ON THE HOST from the compact blob (GpuShardEngine(host_results=True): packed at the end of the pass, copied
        by the copy stream while later passes run): a pipeline.HostBits whose views are valid until three passes later.  Rows, bits,
        pauses and offsets are the rank's LOCAL piece, as in `piece()`."""
        if self._host is None:
            raise ValueError("the engine was not asked for host results (host_results=True)")
        if not isinstance(self._host, HostBits):
            eng, slot, copied, pass_no = self._host
            self._host = eng._finish_host_copy(slot, copied, self.params, self.qad, pass_no)
        return self._host

    # `stitch` accepts mappings: make the result itself usable as a piece
    def __getitem__(self, k):
        if not hasattr(self, "_piece"):
            self._piece = self.piece()
        return self._piece[k]


class GpuShardEngine(DevicePipeline):
    """DevicePipeline (context, stream, output buffers) + the shard phases.
    host_results=True: every pass also leaves its compact result blob (include/urhgpu.h) in pinned
    host memory -- packed at the end of the pass's tail, copied by a third stream while the following passes run, three blob slots in
    rotation, the copy sized by the previous pass's blob (what a prediction misses is fetched when the result is looked at):
    ShardResult.host().  The same window as the single-GPU CaptureStream, per rank."""

    def __init__(self, device: int = 0, pipelined: bool = False, tuning=None, tail_stream_priority: int = 0, host_results: bool = False,
                 worst_case_rows: bool = False):
        """worst_case_rows: size the pulse table for one row per (tolerance + 1) samples (a shard of noise) instead of the default
        four rows per symbol, which a pass that needs more reports as ERR_CAPACITY"""
        super().__init__(device, pipelined=pipelined, tuning=tuning, tail_stream_priority=tail_stream_priority)
        self.worst_case_rows = bool(worst_case_rows)
        self.host_results = bool(host_results)
        self._pass = 0
        self._hslots = None                                 # [(device blob, pinned host blob, copy-done event)] x 3
        self._copy_stream = None
        self._predicted = 0                                 # bytes the next copy is sized for (0: the whole blob)
        self._hqueued = [False, False, False]               # a copy has been queued for the slot (its event means something)
        self._slot_pass = [-1, -1, -1]                      # the pass whose blob the slot holds: a result looked at too late says so

    def _host_slot(self, cap_rows, cap_bits, cap_msg, cap_pos, has_pos):
        torch = self.torch
        cap = int(_lib.load().urhgpu_blob_capacity(cap_rows, cap_bits, cap_msg, cap_pos, 1 if has_pos else 0))
        if self._hslots is None or self._hslots[0][0].numel() < cap:
            self._hslots = [(torch.empty(cap, dtype=torch.uint8, device=self.device), torch.empty(cap, dtype=torch.uint8).pin_memory(),
                             torch.cuda.Event()) for _ in range(3)]
            self._hevents = [torch.cuda.Event() for _ in range(3)]     # "the pass's tail has packed the blob" (one per slot: no event made per pass)
            self._copy_stream = torch.cuda.Stream(self.device)
            self._predicted = 0
            self._hqueued = [False, False, False]
            self._slot_pass = [-1, -1, -1]                  # (results of earlier passes point at the old buffers: host() on them raises)
        k = self._pass % 3
        self._slot_pass[k] = self._pass
        self._pass += 1
        return k, cap

    def _queue_host_copy(self, k):
        """behind the pass's tail (the current stream), on the copy stream: the first `predicted` bytes of the blob"""
        torch = self.torch
        dblob, hblob, done = self._hslots[k]
        if self._predicted <= 0:
            # nobody has looked at a result yet: size the copy by whichever earlier blob has already arrived (else: the whole slot)
            for j in range(3):
                if j != k and self._hqueued[j] and self._hslots[j][2].query():
                    hdr = self._hslots[j][1][:128].numpy().view(np.int64)
                    if int(hdr[0]) == _lib.BLOB_MAGIC:
                        self._predicted = max(self._predicted, abs(int(hdr[6])) + abs(int(hdr[6])) // 8 + 65536)
        n = dblob.numel() if self._predicted <= 0 else min(dblob.numel(), self._predicted)
        self._hqueued[k] = True
        ev = self._hevents[k]
        ev.record(torch.cuda.current_stream(self.device))
        self._copy_stream.wait_event(ev)
        with torch.cuda.stream(self._copy_stream):
            hblob[:n].copy_(dblob[:n], non_blocking=True)
            done.record(self._copy_stream)
        return n

    def _finish_host_copy(self, k, copied, params, qad, pass_no):
        if self._slot_pass[k] != pass_no:
            raise RuntimeError(f"ShardResult.host(): the blob slot of pass {pass_no} has been reused by pass {self._slot_pass[k]} (three blob slots "
                               f"rotate: look at a result before three later passes have been issued) or the slots were reallocated")
        dblob, hblob, done = self._hslots[k]
        done.synchronize()
        hdr = hblob[:128].numpy().view(np.int64)
        total = abs(int(hdr[6]))
        if total > copied:                                   # the prediction fell short: the rest now
            with self.torch.cuda.stream(self._copy_stream):
                hblob[copied:total].copy_(dblob[copied:total], non_blocking=False)
        self._predicted = total + total // 8 + 65536
        h = HostBits.from_blob(hblob.data_ptr(), params, n_samples=int(qad.shape[0]) if qad is not None else 0,
                               d_qad=qad.data_ptr() if qad is not None else 0)
        h.sharded_piece = True
        return h

    # ---- plumbing shared by the phases ----
    def _rows_view(self, t, what=None, own=True):
        """(n, 2) view of a tensor of a sample type, (n, 2) or complex64 (n,), and its numpy dtype.  what None: the view alone (no dtype).
        what given: shape and sample type are checked and, with own, what else a rank can get wrong about a shard on its own (`_own`)"""
        iq = self.torch.view_as_real(t) if t.dtype == self.torch.complex64 else t
        if what is None:
            return iq, None
        if iq.dim() != 2 or iq.shape[1] != 2:
            raise ValueError("IQ must be an (N, 2) tensor or complex64 (N,)")
        npdt = _torch_dtype(iq)
        if own:
            self._own(iq, what)
        return iq, npdt

    def _own(self, t, what):
        """everything a rank can get wrong about a shard on its own, refused before anything is exchanged"""
        if not t.is_cuda or t.device != self.device:
            raise ValueError(f"{what}: the shard lies on {t.device}, the engine runs on {self.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: the shard must be contiguous")

    def _call(self, fn_name, *args, set_stream=True):
        """one call into the library on this engine's context, its return code checked.  set_stream: the context works on the current torch
        stream; False for the phases of a pass, which keep the streams its `_setup` chose (they run under tail_context)"""
        if set_stream:
            self.ctx.set_stream(self.torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(getattr(_lib.load(), fn_name)(self.ctx.handle, *args))

    def tail(self, iq_local, p):
        return self._rows_view(iq_local)[0][-2:].contiguous()  # (2, 2): samples n-2, n-1

    def halo_view(self, left_halo):
        """(2, 2) view of a caller-provided halo (complex64 (2,) or (2, 2) in the capture's dtype)"""
        left_halo, _ = self._rows_view(left_halo)
        if tuple(left_halo.shape) != (2, 2):
            raise ValueError("left_halo: the two samples before the shard, shape (2, 2)")
        return left_halo.contiguous()

    def fir_tail(self, iq_local, k):
        return self._rows_view(iq_local)[0][-k:].contiguous()

    def fir(self, iq_local, taps, left):
        """complex64 FIR of this shard (float32 (N, 2) or complex64 (N,)) with `left` (the m-1 preceding samples) as history"""
        torch = self.torch
        x, h = self._rows_view(iq_local)[0], self._rows_view(taps)[0]
        if x.dtype != torch.float32 or h.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("FIR needs contiguous float32 / complex64 samples and taps")
        if h.dim() != 2 or h.shape[1] != 2:
            raise ValueError("taps: complex64 (m,) or float32 (m, 2)")          # a flat float32 vector would be read as twice the taps
        h = h.contiguous()
        out = torch.empty_like(x)
        self._call("urhgpu_fir_filter_dev", C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(h.data_ptr()), h.shape[0],
                   C.c_void_p(left.data_ptr()) if left is not None else None, C.c_void_p(out.data_ptr()))
        self._fir_keep = (x, h, left)
        return out if iq_local.dtype != torch.complex64 else torch.view_as_complex(out)

    def _setup(self, iq, p, want_qad, n_total=0):
        torch = self.torch
        iq, _ = self._rows_view(iq)
        if iq.dim() != 2 or iq.shape[1] != 2 or not iq.is_contiguous():
            raise ValueError("IQ must be a contiguous (N, 2) tensor")
        npdt = _torch_dtype(iq)
        n = iq.shape[0]
        cp = p.to_c(npdt)
        cap_rows, cap_bits, cap_msg, cap_pos = self.capacities(n, p, (n // (p.tolerance + 1) + 2) if self.worst_case_rows else None)
        # a rank owns the rows that END in its shard -- one that began in an earlier shard (a stuck carrier across the boundary) -- and, ASK,
        # the equal-state rows of LATER shards merged into its last one: a row can span the whole capture, whatever the shard's size
        extra = (max(int(n_total) - n, 0) // max(int(p.samples_per_symbol), 1) + 1) * int(p.bits_per_symbol)
        cap_bits += extra
        cap_pos += extra
        bufs, o = self._output_set("", n if want_qad else None, (cap_rows, cap_bits, cap_msg, cap_pos), p.write_bit_sample_pos)
        pos = bufs[5]
        self._hslot = None
        if self.host_results:
            k, cap = self._host_slot(cap_rows, cap_bits, cap_msg, cap_pos if pos is not None else 0, pos is not None)
            dblob, _, done = self._hslots[k]
            # the blob slot is written by this pass's tail: behind the copy that last read it (three passes ago)
            (self.tail_stream if self.tail_stream is not None else torch.cuda.current_stream(self.device)).wait_event(done)
            o.blob = dblob.data_ptr(); o.cap_blob = cap
            self._hslot = k
        self._res = ShardResult(*bufs, p, self.ctx)
        self._ask = p.modulation_type == "ASK"
        self._keep = (iq,)                                     # keep the inputs alive until the pass is over
        # here and not at every phase: the phases behind the hot launch run under tail_context, where the current stream is the tail stream
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self._pre = (iq, n, cp, o)                             # the pass as set up, until `runs` takes it
        return self._pre

    def runs_begin(self, iq, pos_base, n_total, rank, world, p, want_qad):
        """start the hot kernel on every chunk but the first while the halo all-gather is still in flight"""
        iq, n, cp, o = self._setup(iq, p, want_qad, n_total)
        self._call("urhgpu_shard_prelaunch_dev", C.c_void_p(iq.data_ptr()), n, int(pos_base), int(n_total), int(rank), int(world), C.byref(cp),
                   C.byref(o), set_stream=False)

    def runs_launch(self, iq, left, pos_base, n_total, rank, world, p, want_qad):
        """the whole hot launch: the halo came with the shard (no exchange)"""
        iq, n, cp, o = self._setup(iq, p, want_qad, n_total)
        self._keep += (left,)
        self._call("urhgpu_shard_launch_dev", C.c_void_p(iq.data_ptr()), n, int(pos_base), int(n_total), int(rank), int(world),
                   C.c_void_p(left.data_ptr()) if left is not None else None, C.byref(cp), C.byref(o), set_stream=False)

    def runs(self, iq, left, pos_base, n_total, rank, world, p, want_qad):
        torch = self.torch
        if getattr(self, "_pre", None) is None:                 # no hot launch, Costas or demodulation phase has set the pass up
            self._setup(iq, p, want_qad, n_total)
        (iq, n, cp, o), self._pre = self._pre, None
        self._keep += (left,)
        if left is not None and getattr(self, "tail_stream", None) is not None:
            left.record_stream(self.tail_stream)                # gathered under the caller's stream, read by the first chunk on the tail stream
        summary = self._buf("summary", (9,), torch.int64)      # URHGPU_SHARD_SUMMARY_BYTES = 72
        lh = C.c_void_p(left.data_ptr()) if left is not None else None
        self._call("urhgpu_shard_runs_dev", C.c_void_p(iq.data_ptr()), n, int(pos_base), int(n_total), int(rank), int(world), lh, C.byref(cp),
                   C.byref(o), C.c_void_p(summary.data_ptr()), set_stream=False)
        return summary

    # ---- PSK: the Costas loop across shards (sharding/costas.py, steps 1-4; include/urhgpu.h) ----
    def costas_spec(self, iq_local, left_raw, pos_base, n_total, rank, world, p):
        """speculate the shard (its first chunk warms up in left_raw, the raw samples before it; None on rank 0) -> the summary
        (uint8 device tensor of COSTAS_SUMMARY_BYTES)"""
        from .sharding import COSTAS_SUMMARY_BYTES
        torch = self.torch
        if self.tail_stream is not None:
            raise ValueError("PSK shards run on an engine that is not pipelined: GpuShardEngine(pipelined=False)")
        iq, n, cp, o = self._setup(iq_local, p, True, n_total)    # the qad always: the runs phase segments it
        halo = None
        if left_raw is not None:
            halo, _ = self._rows_view(left_raw)
            if halo.dtype != iq.dtype or halo.dim() != 2 or halo.shape[1] != 2:
                raise ValueError("left_raw: raw samples in the shard's dtype, (m, 2) or complex64 (m,)")
            halo = halo.contiguous()
            self._keep += (halo,)
        summary = self._buf("costas_summary", (COSTAS_SUMMARY_BYTES,), torch.uint8)
        self._costas_end = self._buf("costas_end", (2,), torch.int32)
        self._costas_end.zero_()
        self._call("urhgpu_shard_costas_spec_dev", C.c_void_p(iq.data_ptr()), n, int(pos_base), int(n_total), int(rank), int(world),
                   C.c_void_p(halo.data_ptr()) if halo is not None else None, int(halo.shape[0]) if halo is not None else 0,
                   C.byref(cp), C.byref(o), C.c_void_p(summary.data_ptr()), set_stream=False)
        return summary

    def costas_resolve(self, start):
        """stitch the shard from its true start state (freq bits, phase bits) and write its qad"""
        st = (C.c_uint32 * 2)(int(start[0]), int(start[1]))
        self._call("urhgpu_shard_costas_resolve_dev", st, C.c_void_p(self._costas_end.data_ptr()), set_stream=False)

    def costas_end(self):
        """the shard's true end state (2 x int32: float32 bits) once it has resolved, zeros before"""
        return self._costas_end

    def costas_last(self):
        """the shard's last demodulated value (1 float): the next rank's halo of the pulse table"""
        return self._res.qad[-1:]

    def costas_stats(self):
        return self.ctx.costas_stats()

    def costas_qad(self):
        """the shard's demodulated signal (float32 (n_local,)) once it has resolved: what an auto-center pass estimates from"""
        return self._res.qad

    def set_center(self, center):
        """the center the pass's remaining phases (the pulse table) use instead of the parameters' own"""
        self._pre[2].center = float(center)

    # ---- ASK / FSK: the demodulation phase on its own (sharding/pipeline.py: iq_to_bits_auto; urhgpu_shard_demod_dev) ----
    def demod_own(self, iq_local, left_halo=None):
        """everything a rank can get wrong about the arguments of a pass that demodulates first, on its own: refused before anything is
        exchanged (shape, sample type, device, contiguity, the halo handed over with the shard, a pipelined engine)"""
        if self.tail_stream is not None:
            raise ValueError("a pass that demodulates first runs on an engine that is not pipelined: GpuShardEngine(pipelined=False) "
                             "(gathered values are read on the host between its phases)")
        iq, _ = self._rows_view(iq_local, "iq_to_bits_auto")
        if left_halo is not None:
            halo = self.halo_view(left_halo)
            if halo.dtype != iq.dtype or halo.device != iq.device:
                raise ValueError("left_halo: the two samples before the shard, in the shard's sample type and on its device")

    def demod(self, iq_local, left, pos_base, n_total, rank, world, p):
        """demodulate the shard once into the result's qad (left: the two raw samples before it, None on rank 0) and leave the seam value
        -- the demodulated value of the sample before the shard -- on the device: `runs` then segments the qad"""
        iq, n, cp, o = self._setup(iq_local, p, True, n_total)
        self._keep += (left,)
        self._call("urhgpu_shard_demod_dev", C.c_void_p(iq.data_ptr()), n, int(pos_base), int(n_total), int(rank), int(world),
                   C.c_void_p(left.data_ptr()) if left is not None else None, C.byref(cp), C.byref(o), set_stream=False)

    def demod_qad(self):
        """the shard's demodulated signal (float32 (n_local,)) once `demod` has run: what an auto-center pass estimates from"""
        return self._res.qad

    def demod_seam(self):
        """the seam value of the last `demod` on a rank > 0, read back (a numpy float32): tests and diagnostics"""
        v = (C.c_float * 1)()
        self._call("urhgpu_shard_seam_value", v, set_stream=False)
        return np.frombuffer(v, dtype=np.float32)[0].copy()        # (the bits as they are: no trip through a Python float)

    # ---- the estimators' partial reductions (sharding/pipeline.py: detect_noise_level / detect_center; csrc/shard_estimators.hip) ----
    def noise_partials(self, iq_local, pos_base, n_total, chunk, n_chunks):
        """float64 (2, n_chunks): fp64 sum and max of the magnitudes of the intersection of every chunk with the shard"""
        from .signal_functions import dtype_code
        iq, npdt = self._rows_view(iq_local, "detect_noise_level")
        out = self.torch.empty((2, int(n_chunks)), dtype=self.torch.float64, device=self.device)
        if n_chunks:
            self._call("urhgpu_magnitude_chunk_partials_dev", C.c_void_p(iq.data_ptr()), dtype_code(npdt), int(iq.shape[0]), int(pos_base),
                       int(n_total), int(chunk), int(n_chunks), C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
        out._urh_keep = iq
        return out

    def compact_gt(self, x, thr):
        """x[x > thr], order kept -> (float32 tensor of len(x) whose first `count` elements are the kept ones, int64 (1,) count)"""
        torch = self.torch
        if x.dtype != torch.float32 or x.dim() != 1:
            raise ValueError("detect_center: a float32 1-D tensor (the shard's demodulated signal)")
        self._own(x, "detect_center")
        n = int(x.shape[0])
        kept = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._call("urhgpu_compact_gt_dev", C.c_void_p(x.data_ptr()), n, float(thr), C.c_void_p(kept.data_ptr()), C.c_void_p(cnt.data_ptr()))
        kept._urh_keep = x
        return kept, cnt

    def pairwise_partial(self, x, g_off, m_total, mode, mean, words):
        """the record of urhgpu_pairwise_partial_f32_dev for x = elements [g_off, g_off + len(x)) of a sequence of m_total, padded with
        zeros to `words` float32 (every rank gathers the same shape)"""
        rec = self.torch.zeros(int(words), dtype=self.torch.float32, device=self.device)
        n_out = C.c_int64(0)
        self._call("urhgpu_pairwise_partial_f32_dev", C.c_void_p(x.data_ptr()) if x.numel() else None, int(x.shape[0]), int(g_off), int(m_total),
                   int(mode), float(mean), C.c_void_p(rec.data_ptr()), int(words), C.byref(n_out))
        rec._urh_keep = x
        return rec

    def histogram(self, x, edges):
        """np.histogram(x, bins=edges) of the rank's elements: int64 (len(edges) - 1,) on the device"""
        torch = self.torch
        d_edges = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(self.device)
        counts = torch.empty(len(edges) - 1, dtype=torch.int64, device=self.device)
        self._call("urhgpu_histogram_f32_dev", C.c_void_p(x.data_ptr()) if x.numel() else None, int(x.shape[0]), C.c_void_p(d_edges.data_ptr()),
                   len(edges), C.c_void_p(counts.data_ptr()))
        counts._urh_keep = (x, d_edges)
        return counts

    # ---- DC correction across the shards (sharding/pipeline.py: dc_correct; csrc/dc_correct.hip, "sharded captures") ----
    def _dc_rows(self, t, what):
        """(n, 2) view of a tensor of a sample type or complex64 (n,), and its dtype code"""
        from .filter import _TORCH_CODES
        x, _ = self._rows_view(t)
        code = _TORCH_CODES.get(str(x.dtype))
        if code is None:
            raise ValueError(f"{what}: Unsupported dtype {x.dtype}")
        if x.dim() != 2 or x.shape[1] != 2:
            raise ValueError(f"{what}: an (n, 2) tensor of a sample type or complex64 (n,)")
        return x, code

    def dc_own(self, iq_local, also, out):
        """everything a rank can get wrong about the arguments of dc_correct on its own -> is the capture float32"""
        x, code = self._dc_rows(iq_local, "dc_correct")
        self._own(x, "dc_correct")
        if out is not None and out is not iq_local:
            raise ValueError("dc_correct: out is None or the shard itself")
        for t in also:
            a, a_code = self._dc_rows(t, "dc_correct: also")
            if a_code != code:
                raise ValueError("dc_correct: `also` holds tensors of the shard's sample type")
            self._own(a, "dc_correct: also")
        return code == _lib.DT_F32

    def dc_whole(self, iq_local, out):
        """one rank: the single-GPU function -> (the corrected capture, its mean on the host)"""
        from .filter import dc_correct_dev
        res, mean = dc_correct_dev(self, iq_local, out=out, want_mean=True)
        self._dc_single = self._dc_rows(iq_local, "dc_correct")[1] == _lib.DT_F32
        return res, mean.cpu().numpy()

    def dc_sums(self, iq_local):
        """int64 (3,): n_local and the two column sums (float32 captures: the bits of two float64 sums)"""
        x, code = self._dc_rows(iq_local, "dc_correct")
        words = self.torch.empty(3, dtype=self.torch.int64, device=self.device)
        self._call("urhgpu_shard_dc_sums_dev", C.c_void_p(x.data_ptr()) if x.shape[0] else None, int(x.shape[0]), code, C.c_void_p(words.data_ptr()))
        words._urh_keep = x
        self._dc_single = None
        return words

    def dc_spec(self, iq_local, base):
        """int32 (2, 2, 4): the shard's records [column][path] {entry, exit, room, flags}, speculated from the float64 sums in front"""
        x, _ = self._dc_rows(iq_local, "dc_correct")
        recs = self.torch.empty((2, 2, 4), dtype=self.torch.int32, device=self.device)
        self._call("urhgpu_shard_dc_spec_dev", C.c_void_p(x.data_ptr()) if x.shape[0] else None, int(x.shape[0]),
                   (C.c_double * 2)(float(base[0]), float(base[1])), C.c_void_p(recs.data_ptr()))
        recs._urh_keep = x
        return recs

    def dc_resolve(self, iq_local, entry):
        """int32 (2,): the bits of the shard's exits when entered with `entry` (bits I, bits Q); entry None: zeros, for the ranks that only
        take part in the hand-over"""
        out = self.torch.zeros(2, dtype=self.torch.int32, device=self.device)
        if entry is not None:
            x, _ = self._dc_rows(iq_local, "dc_correct")
            self._call("urhgpu_shard_dc_resolve_dev", C.c_void_p(x.data_ptr()) if x.shape[0] else None, int(x.shape[0]),
                       (C.c_uint32 * 2)(int(entry[0]), int(entry[1])), C.c_void_p(out.data_ptr()))
            out._urh_keep = x
        return out

    def dc_apply(self, t, mean, out=None):
        """t minus the mean (host: two float32 for float32 samples, two float64 otherwise), into a new tensor or t itself"""
        x, code = self._dc_rows(t, "dc_correct")
        res = self.torch.empty_like(t) if out is None else out
        y, _ = self._rows_view(res)
        m = np.ascontiguousarray(mean, dtype=np.float32 if code == _lib.DT_F32 else np.float64)
        self._call("urhgpu_shard_dc_apply_dev", C.c_void_p(x.data_ptr()) if x.shape[0] else None, int(x.shape[0]), code, C.c_void_p(m.ctypes.data),
                   C.c_void_p(y.data_ptr()) if x.shape[0] else None)
        res._urh_keep = x
        return res

    def dc_stats(self):
        """this rank's stitches of the last dc_correct: chunks per column, chunks derived from their records, chunks re-evaluated serially"""
        st = (C.c_int64 * 8)()
        single = getattr(self, "_dc_single", None)
        if single is not None:
            if single:
                self._call("urhgpu_test_dc_stats", st, set_stream=False)
            return {"chunks": int(st[0]), "derived": int(st[1]), "reevaluated": int(st[2])}
        self._call("urhgpu_shard_dc_stats", st, set_stream=False)
        return {"chunks": int(st[0]), "derived": int(st[1] + st[5]), "reevaluated": int(st[2] + st[6])}

    # ---- message records across the shards (sharding/pipeline.py: message_records; csrc/msg_records.hip, "sharded capture") ----
    def _records_outputs(self, res):
        """the C descriptor of a ShardResult's buffers: what the records kernels read of the pass (positions required)"""
        if res.pos_buf is None:
            raise ValueError("message_records needs the positions of the pass (write_bit_sample_pos)")
        return self._outputs(None, res.rows_buf, res.bits_buf, res.msg_off_buf, res.pauses_buf, res.pos_buf, res.pos_off_buf, res.counts)

    def records_summary(self, iq_local, res, pos_base):
        """int64 (REC_SUMMARY_WORDS,): this rank's summary words, from the pass's device counts and offsets (nothing read back)"""
        from .sharding import REC_SUMMARY_WORDS
        iq, _ = self._rows_view(iq_local, "message_records")   # everything a rank can get wrong on its own, before anything is exchanged
        o = self._records_outputs(res)
        words = self.torch.empty(REC_SUMMARY_WORDS, dtype=self.torch.int64, device=self.device)
        self._call("urhgpu_shard_records_summary_dev", int(iq.shape[0]), int(pos_base), C.byref(o), C.c_void_p(words.data_ptr()))
        return words

    def records_lookup(self, res, index):
        """int64 (len(index),): the position entries asked of this rank (index: local indices, -1 where another rank holds the entry)"""
        torch = self.torch
        o = self._records_outputs(res)
        d_index = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).to(self.device)
        values = torch.empty(len(index), dtype=torch.int64, device=self.device)
        self._call("urhgpu_shard_records_lookup_dev", C.byref(o), C.c_void_p(d_index.data_ptr()), len(index), C.c_void_p(values.data_ptr()))
        values._urh_keep = d_index
        return values

    def records_window_part(self, iq_local, pos_base, spans, w_max):
        """uint8 (len(spans), w_max, bytes per sample): of every window [lo, lo + w) asked for, the raw samples this shard holds, in their
        place; zeros elsewhere (plumbing: slices of the shard)"""
        torch = self.torch
        iq, npdt = self._rows_view(iq_local, "message_records")
        raw = iq.view(torch.uint8).view(int(iq.shape[0]), 2 * npdt.itemsize)
        part = torch.zeros((len(spans), int(w_max), 2 * npdt.itemsize), dtype=torch.uint8, device=self.device)
        a0, b0 = int(pos_base), int(pos_base) + int(iq.shape[0])
        for j, (lo, w) in enumerate(spans):
            a, b = max(lo, a0), min(lo + w, b0)
            if b > a:
                part[j, a - lo:b - lo] = raw[a - a0:b - a0]
        return part

    def records_finish(self, iq_local, res, pos_base, n_total, p, divisor, first, window):
        """the records kernel -> this rank's records on the host (protocol.RECORD_DTYPE, one per message closed here)"""
        from .protocol import RECORD_DTYPE
        torch = self.torch
        iq, npdt = self._rows_view(iq_local, "message_records")
        o, cp = self._records_outputs(res), p.to_c(npdt)
        cap = max(int(o.cap_msg), 1)
        d_rec = self._buf("shard_records", (cap * RECORD_DTYPE.itemsize,), torch.uint8)
        block = self._pinned_block(("records", "shard"), cap * RECORD_DTYPE.itemsize)
        first = np.ascontiguousarray(first, dtype=np.int64)
        if window is not None:
            window = window.contiguous()
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)      # the read-back below waits on this stream
        self._call("urhgpu_shard_msg_records_dev", C.c_void_p(iq.data_ptr()), int(iq.shape[0]), int(pos_base), int(n_total), C.byref(cp), C.byref(o),
                   int(divisor), first.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(window.data_ptr()) if window is not None else None,
                   int(window.shape[0]) if window is not None else 0, C.c_void_p(d_rec.data_ptr()), cap, C.c_void_p(block.data_ptr()),
                   set_stream=False)
        n_msg = min(int(res.counts[1:2].cpu()[0]), cap)       # waits for the kernels: the shard and the window are free again, the mirror is complete
        return block.numpy().view(RECORD_DTYPE)[:n_msg].copy()

    def rows(self, summaries):
        torch = self.torch
        self._keep += (summaries,)
        merge = self._buf("merge", (5,), torch.int64) if self._ask else None
        self._call("urhgpu_shard_rows_dev", C.c_void_p(summaries.data_ptr()), C.c_void_p(merge.data_ptr()) if merge is not None else None,
                   set_stream=False)
        return merge

    def bits_prepare(self, merged_all):
        torch = self.torch
        self._keep += (merged_all,)
        flags = self._buf("flags", (3,), torch.int64)
        self._call("urhgpu_shard_bits_prepare_dev", C.c_void_p(merged_all.data_ptr()) if merged_all is not None else None,
                   C.c_void_p(flags.data_ptr()), set_stream=False)
        return flags

    def bits_finish(self, flags_all):
        self._keep += (flags_all,)
        self._call("urhgpu_shard_bits_finish_dev", C.c_void_p(flags_all.data_ptr()), set_stream=False)
        if self._hslot is not None:
            self._res._host = (self, self._hslot, self._queue_host_copy(self._hslot), self._slot_pass[self._hslot])
        res, self._res = self._res, None
        res._keep = self._keep
        self._keep = ()
        return res
