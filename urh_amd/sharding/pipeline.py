"""One rank's orchestration of the sharded passes (`ShardedPipeline`), how a capture is cut (`shard_bounds`) and how the ranks' pieces
become the flat result (`stitch`).  The fused ASK / FSK pass exchanges a halo, a summary, (ASK) a merge row and three flags: the package
docstring has the table.  PSK: costas.py.  DC correction: dc.py.  Message records: records.py.

Estimators: `detect_noise_level` and `detect_center` of the whole capture from the ranks' shards -- partial reductions per rank and small
all-gathers (one for the noise level; four for the center: kept counts, two records of numpy's float32 pairwise sum evaluated from the
rank's global offset, histogram counts), every result a pure function of gathered data (pairwise.py).  A PSK pass detects its own center
with `auto_center=True`.

Automatic passes: `iq_to_bits_auto(auto_noise=..., auto_center=...)` opens a sharded capture the way DevicePipeline.iq_to_bits(auto_noise=True,
auto_center=True) opens one on a single GPU -- the reference's defaults -- with the same bits.  auto_noise: `detect_noise_level` first (one
all-gather more), the pass gates with its value; where that is not below the sample type's max_magnitude every rank raises ValueError, decided
from the gathered value.  auto_center, PSK: as above.  auto_center, ASK and FSK -- whose fused hot kernel needs the center before the
demodulated signal exists -- take a route of their own that demodulates every shard ONCE:

    1. halo        as in the fused pass (or handed over with the shard: halo_given)
    2. demodulate  the shard into the result's qad (urhgpu_shard_demod_dev: the demodulation-only kernels), and from the halo's two raw samples
                   the SEAM VALUE: the demodulated value of the sample before the shard, kept on the device
    3. center      `detect_center` of the ranks' demodulated signals (four all-gathers at most); p.center where it finds none
    4. summary / rows / flags as in the fused pass, the runs segmented from the qad with that center (the qad-input kernels of the PSK pass),
                   the seam value being the left halo: the ranks do not exchange their last demodulated values

The route reads gathered values on the host and therefore refuses a pipelined engine, like PSK.  `last_auto` records the noise level, the
center, whether it was detected, and the number of all-gathers.

The orchestration is engine-agnostic: `engine` is the GPU engine (urh_amd.shard_engine.GpuShardEngine, HIP kernels behind the C ABI) in
production; the CPU test-suite drives the same orchestration with the executable model of the kernels (tests/model_shard.py) over a
world_size-2 gloo group and over ThreadComm."""
import contextlib

import numpy as np

from .comm import _CountingComm, carry_across_ranks
from .costas import costas_exchange, costas_halo_samples
from .dc import dc_compose
from .pairwise import HIST_GATHER_BINS, center_parts, minmax_combine, pairwise_combine, pairwise_record_words
from .records import REC_FIRST_WORDS, REC_N_LOCAL, REC_POS_BASE, REC_SUMMARY_WORDS, records_plan, records_requests, records_windows


def shard_bounds(n_total: int, world: int):
    """[begin, end) of every rank's shard: equal shards of ceil(n/world) samples rounded up to a multiple of
    64 (so that every shard starts 16-byte aligned for every IQ dtype), the last rank takes what is left.
    Every shard needs >= 2 samples."""
    per = -(-n_total // world)
    per = -(-per // 64) * 64
    b = [min(r * per, n_total) for r in range(world + 1)]
    b[world] = n_total
    if any(b[r + 1] - b[r] < 2 for r in range(world)):
        raise ValueError(f"capture of {n_total} samples is too short to shard over {world} ranks")
    return [(b[r], b[r + 1]) for r in range(world)]


class ShardedPipeline:
    """One rank's view of the sharded IQ->bits pass."""

    def __init__(self, engine, comm):
        self.engine, self.comm = engine, comm
        self.rank, self.world = comm.rank, comm.world
        self.last_costas = None                  # PSK: the last pass's Costas exchange (rounds, this rank's chunks by map / checkpoint / serial)
        self.last_center = None                  # the center the last pass's pulse table was built with (auto_center: the detected one)
        self.last_dc = None                      # the last dc_correct: mean, all-gathers, this rank's stitch statistics
        self.last_records = None                 # the last message_records: all-gathers, windows exchanged
        self.last_auto = None                    # the last iq_to_bits_auto: noise, center, center_detected, all_gathers
        self._center_found = False               # the last pass's pulse table was built with a center it detected

    # bench.py / DevicePipeline compatible surface ------------------------------------------------
    @property
    def ctx(self):
        return self.engine.ctx

    def reserve(self, n_local, p):
        self.engine.reserve(n_local, p)

    # the steps the passes share ---------------------------------------------------------------------
    def _shard_range(self, iq_local, pos_base, n_total, what=None):
        """(n_local, pos_base, n_total) with the defaults of equal shards of len(iq_local); what given: a shard outside the capture is refused"""
        n_local = int(iq_local.shape[0])
        pos_base = self.rank * n_local if pos_base is None else int(pos_base)
        n_total = self.world * n_local if n_total is None else int(n_total)
        if what is not None and (pos_base < 0 or pos_base + n_local > n_total):
            raise ValueError(f"{what}: the shard does not lie inside the capture")
        return n_local, pos_base, n_total

    @contextlib.contextmanager
    def _counting(self):
        """self.comm counts the all-gathers that pass through it, whichever method enters them -> the counting wrapper"""
        counted = _CountingComm(self.comm)
        self.comm, comm = counted, self.comm
        try:
            yield counted
        finally:
            self.comm = comm

    def _left_halo(self, halo_given, left_halo, view=True):
        """halo_given: a rank > 0 without its halo is refused; view: the halo as the engine takes it (None on rank 0 or without halo_given)"""
        if halo_given and self.rank > 0 and left_halo is None:
            raise ValueError("halo_given: ranks > 0 pass the two samples before their shard as left_halo")
        if not (view and halo_given and self.rank > 0):
            return None
        return self.engine.halo_view(left_halo) if hasattr(self.engine, "halo_view") else left_halo

    def _check_psk_own(self, p, pos_base, n_total, left_raw, auto_center):
        """everything a rank can get wrong about a PSK pass on its own -> the raw samples before the shard, cut to the ones the pass reads"""
        if auto_center:
            self._estimator_engine("costas_qad", "set_center", "compact_gt", "pairwise_partial", "histogram")
        if n_total <= 2:
            raise ValueError("PSK: a capture of two samples or fewer does not shard")
        if self.rank == 0:
            return None
        need = costas_halo_samples(p.costas_loop_bandwidth, pos_base)
        have = 0 if left_raw is None else int(left_raw.shape[0])
        if have < need:
            raise ValueError(f"PSK: rank {self.rank} needs the {need} raw samples before its shard as left_raw (got {have})")
        return left_raw[have - need:]

    def _table_tail(self, iq_local, left, pos_base, n_total, p, want_qad):
        """summary / rows / (ASK) merge / flags / finish: the shard's runs to this rank's piece of the result, three (ASK: four) phases with
        an all-gather between them"""
        e, c = self.engine, self.comm
        summary = e.runs(iq_local, left, pos_base, n_total, self.rank, self.world, p, want_qad)
        merge = e.rows(c.all_gather(summary))
        flags = e.bits_prepare(c.all_gather(merge) if merge is not None else None)
        return e.bits_finish(c.all_gather(flags))

    def fir_filter(self, iq_local, taps, left_raw=None, want_halo=False, raw_halo=None):
        """Signal.filter_range semantics on a sharded capture (BASELINE.json configs[3], "FIR-halo exchange"): every rank
        filters its shard with the m-1 samples that precede it as history; rank 0 starts from zero history like the
        reference's fir_filter (signal_functions.pyx:513-525).  Returns the filtered shard (same shape as iq_local -- also for empty
        taps, where the reference's host function drops one sample: n - 1 zeros).
        left_raw is None: the history is the left neighbour's tail, one all-gather of (m-1) * 8 bytes per rank.
        left_raw given (every rank but the first; round 5): whoever distributed the capture handed the rank the m + 1 RAW samples
        that precede its shard ((m + 1, 2) float32 / complex64 (m + 1,): 520 bytes for 64 taps) -- no exchange at all: the last
        m - 1 of them are the filter's history, and filtering the m + 1 themselves gives, in their last two outputs, the two FILTERED
        samples before the shard, i.e. the demodulation's halo (want_halo=True: returns (filtered shard, that halo or None)).
        raw_halo states the mode and must be THE SAME ON EVERY RANK (a rank that guessed it from its own arguments could skip a
        collective the others enter): True = raw mode (rank 0 passes no left_raw, every other rank must), False = exchange,
        None = raw mode iff want_halo (the halo only exists in raw mode; left_raw without want_halo also selects it on ranks > 0,
        where rank 0 then has to say raw_halo=True)."""
        e, c = self.engine, self.comm
        if raw_halo is None:
            raw_halo = bool(want_halo) or left_raw is not None
        m = int(taps.shape[0])                     # complex64 (m,) or float32 (m, 2): rows = taps
        if m <= 1 or self.world == 1:
            out = e.fir(iq_local, taps, None)
            return (out, None) if want_halo else out
        if int(iq_local.shape[0]) < m - 1:
            raise ValueError("shard shorter than the filter history")
        if want_halo and not raw_halo:
            raise ValueError("want_halo needs raw_halo: the filtered halo comes from the raw samples handed over with the shard")
        if raw_halo:
            if self.rank == 0:
                out = e.fir(iq_local, taps, None)
                return (out, None) if want_halo else out
            if left_raw is None:
                raise ValueError("raw_halo: ranks > 0 pass the m + 1 raw samples that precede their shard as left_raw")
            raw = left_raw
            if hasattr(e, "torch") and raw.dtype == e.torch.complex64:
                raw = e.torch.view_as_real(raw)
            if int(raw.shape[0]) != m + 1:
                raise ValueError("left_raw: the m + 1 raw samples that precede the shard")
            out = e.fir(iq_local, taps, raw[2:].contiguous())
            if not want_halo:
                return out
            return out, e.fir(raw.contiguous(), taps, None)[-2:].contiguous()     # outputs m - 1 and m have their full history inside `raw`
        tails = c.all_gather(e.fir_tail(iq_local, m - 1))
        return e.fir(iq_local, taps, tails[self.rank - 1] if self.rank > 0 else None)

    # the estimators that feed the pipelines: partial reductions per rank + small all-gathers -------------------
    def _estimator_engine(self, *names):
        missing = [n for n in names if not hasattr(self.engine, n)]
        if missing:
            raise NotImplementedError(f"the engine offers no {', '.join(missing)}")
        return self.engine

    def detect_noise_level(self, iq_local, pos_base=None, n_total=None):
        """AutoInterpretation.detect_noise_level(get_magnitudes(capture)) (AutoInterpretation.py:60-91) for the capture whose shard
        [pos_base, pos_base + n_local) this rank holds; pos_base / n_total default as in iq_to_bits.  The chunk geometry is the
        capture's (estimators.noise_chunks(n_total): chunks counted from the end, the front remainder dropped): a chunk may straddle
        any number of shards.  Every rank reduces the intersection of every chunk with its shard to an fp64 sum and a max
        (urhgpu_magnitude_chunk_partials_dev), ONE all-gather moves 2 * n_chunks doubles per rank, and every rank adds the sums in
        rank order and folds the maxima (a NaN stays) before the decision of the single-GPU function.  A capture of three samples or
        fewer gives 0 without a collective; on one rank the value is detect_noise_level_dev's.
        The sums are fp64 sums in another order than numpy's pairwise one ("detect_noise_level"): the float32-cast chunk
        means agree with numpy's unless an fp64 sum lies within an ulp of a float32 rounding boundary."""
        from ..estimators import noise_chunks, noise_level_from_chunk_stats
        e, c = self._estimator_engine("noise_partials"), self.comm
        _, pos_base, n_total = self._shard_range(iq_local, pos_base, n_total, "detect_noise_level")
        chunk, n_chunks = noise_chunks(n_total) if n_total > 3 else (1, 0)
        part = e.noise_partials(iq_local, pos_base, n_total, chunk, n_chunks)     # checks the shard before anything is exchanged
        if n_total <= 3:                                                          # :61-62
            return 0
        both = np.asarray(c.all_gather(part).cpu().numpy(), dtype=np.float64).reshape(self.world, 2, n_chunks)
        sums = np.zeros(n_chunks, np.float64)
        for r in range(self.world):
            sums = sums + both[r, 0]
        maxs = both[:, 1].max(axis=0)                                             # np.max: a NaN stays, as within a rank
        return noise_level_from_chunk_stats(sums, maxs, chunk)

    def detect_center(self, qad_local, max_size=None):
        """AutoInterpretation.detect_center(qad, max_size) (AutoInterpretation.py:226-277) where qad is the concatenation of the ranks'
        qad_local (float32, 1-D, on the rank's device) in rank order: bit-equal to estimators.detect_center_dev on the whole signal,
        None on every rank where that gives None.  max_size must be the same on every rank.  Four all-gathers at most:
            1. the kept counts of the local compaction qad > -4 -> the trim [int(0.05 K), int(0.95 K)) and every rank's part of it
            2. the records of np.mean's float32 sum (urhgpu_pairwise_partial_f32_dev, which also takes min / max in that pass)
            3. the records of np.var's second sum, (x - mean)^2 in float32
            4. the int64 counts of np.histogram over the edges every rank computes from the same scalars (more than HIST_GATHER_BINS
               bins -- a nearly constant signal -- go in blocks of that many)
        The sums are numpy's float32 pairwise sums bit for bit (pairwise_combine finishes what the shard boundaries cut).  Every
        early return is decided from gathered data."""
        from ..estimators import peaks_center
        e, c = self._estimator_engine("compact_gt", "pairwise_partial", "histogram"), self.comm
        if max_size is not None and int(max_size) < 0:
            raise ValueError("detect_center: max_size must not be negative")
        kept, cnt = e.compact_gt(qad_local, -4.0)                                 # checks the shard before anything is exchanged
        counts = c.all_gather(cnt).cpu().numpy().reshape(-1)
        m, parts = center_parts(counts, max_size)
        if m == 0:
            return None             # np.var of an empty slice is nan -> np.arange raises ValueError -> None (:246-248)
        begin, g_r, m_r = parts[self.rank]
        mine = kept[begin:begin + m_r]
        words = max(pairwise_record_words(g, k, m) for _, g, k in parts)
        recs = c.all_gather(e.pairwise_partial(mine, g_r, m, 0, 0.0, words)).cpu().numpy()
        hist_min, hist_max = minmax_combine(recs)
        with np.errstate(all="ignore"):
            mean = pairwise_combine(recs, m) / np.float32(m)                      # np.mean: float32 sum / float32 count
            recs = c.all_gather(e.pairwise_partial(mine, g_r, m, 1, float(mean), words)).cpu().numpy()
            hist_step = float(pairwise_combine(recs, m) / np.float32(m))          # float(np.var(rect)) (:240)
        try:
            with np.errstate(all="ignore"):
                edges = np.arange(hist_min, hist_max + hist_step, hist_step)      # :243-245
            if len(edges) < 2:
                return None         # np.histogram with fewer than 2 edges raises ValueError -> None (:246-248)
        except (ZeroDivisionError, ValueError):
            return None
        local = e.histogram(mine, edges)
        n_bins = len(edges) - 1
        total = np.zeros(n_bins, np.int64)
        for b0 in range(0, n_bins, HIST_GATHER_BINS):
            b1 = min(n_bins, b0 + HIST_GATHER_BINS)
            total[b0:b1] = c.all_gather(local[b0:b1]).cpu().numpy().reshape(self.world, -1).sum(axis=0)
        return peaks_center(total, edges)

    def dc_correct(self, iq_local, pos_base=None, n_total=None, also=(), out=None):
        """The shard minus the mean of the WHOLE capture: rows [pos_base, pos_base + n_local) of numpy's x - np.mean(x, axis=0) stored into the
        capture's sample type, bit for bit -- the sharded counterpart of filter.dc_correct_dev (dc.py).
        iq_local: (n_local, 2) in one of the five sample types, or complex64 (n_local,); a rank may hold no sample.  pos_base / n_total
        default as in iq_to_bits; the ranks' n_local must add up to n_total (checked from gathered data: every rank raises ValueError).
        also: small tensors of the same sample type corrected with the same mean and returned with the shard -- the raw samples a
        distributor hands over with it (left_halo, the PSK left_raw, the FIR left_raw), without which a corrected shard could not be
        used with halo_given=True, a PSK pass or fir_filter(raw_halo=True).  out: None (a new tensor) or iq_local (in place).
        Returns the corrected shard, or (shard, [corrected also tensors]) when `also` is given.  `last_dc` records the mean (two float64
        for integers, two float32 for float32), the number of all-gathers and this rank's stitch statistics.
        world == 1 is the single-GPU function; n_total == 0 returns the empty shard; neither enters a collective.  The recipe for a
        corrected pass: dc_correct, then iq_to_bits on the result."""
        e = self._estimator_engine("dc_own", "dc_whole", "dc_sums", "dc_spec", "dc_resolve", "dc_apply", "dc_stats")
        also = tuple(also)
        is_f32 = e.dc_own(iq_local, also, out)            # everything a rank can get wrong on its own, before anything is exchanged
        n_local, pos_base, n_total = self._shard_range(iq_local, pos_base, n_total, "dc_correct")
        stats, gathers = {"chunks": 0, "derived": 0, "reevaluated": 0}, 0
        if self.world == 1 and n_local != n_total:
            raise ValueError(f"dc_correct: the ranks hold {n_local} samples, the capture has {n_total}")
        if n_total == 0:
            self.last_dc = {"mean": None, "all_gathers": 0, **stats}
            return (iq_local, list(also)) if also else iq_local
        if self.world == 1:
            res, mean = e.dc_whole(iq_local, out)
            stats = e.dc_stats()
        else:
            with self._counting() as c:
                words = np.ascontiguousarray(c.all_gather(e.dc_sums(iq_local)).cpu().numpy()).view(np.int64).reshape(self.world, 3)
                held = sum(int(v) for v in words[:, 0])
                if held != n_total:                       # decided from gathered data: every rank raises, none is left in a collective
                    raise ValueError(f"dc_correct: the ranks hold {held} samples, the capture has {n_total}")
                if not is_f32:
                    mean = np.array([float(sum(int(v) for v in words[:, k])) / float(n_total) for k in (1, 2)], np.float64)
                else:
                    with np.errstate(all="ignore"):
                        guesses = np.ascontiguousarray(words[:, 1:]).view(np.float64)
                        base = [0.0, 0.0]
                        for r in range(self.rank):
                            base = [base[0] + float(guesses[r, 0]), base[1] + float(guesses[r, 1])]
                        recs = c.all_gather(e.dc_spec(iq_local, base)).cpu().numpy()
                        (_, _, total), _ = carry_across_ranks(
                            c, recs, dc_compose, lambda entries: None,
                            lambda entries, pending: e.dc_resolve(iq_local, entries[pending] if pending == self.rank else None))
                        s = np.array(total, np.uint32).view(np.float32)
                        mean = (s.astype(np.float64) / np.float64(n_total)).astype(np.float32)      # numpy: the float32 sum divided in float64, rounded once
                    stats = e.dc_stats()
            gathers = c.count
            res = e.dc_apply(iq_local, mean, out)
        fixed = [e.dc_apply(t, mean, None) for t in also]
        self.last_dc = {"mean": mean, "all_gathers": gathers, **stats}
        return (res, fixed) if also else res

    def iq_to_bits(self, iq_local, p, want_qad=True, pos_base=None, n_total=None, halo_given=False, left_halo=None, left_raw=None, auto_center=False,
                   msg_records=False, dc_correction=False):
        """iq_local: this rank's shard.  pos_base / n_total default to equal shards of len(iq_local).
        halo_given (the same on every rank): whoever distributed the capture handed every rank but the first the two samples that
        precede its shard (left_halo: (2, 2) in the shard's dtype, or complex64 (2,)) -- 16 bytes more per rank to read from the
        file.  The halo exchange is then skipped: two all-gathers per pass (ASK: three) instead of three (four).
        PSK: every rank but the first passes left_raw, the costas_halo_samples(p.costas_loop_bandwidth, pos_base) raw samples
        before its shard ((m, 2) in the shard's dtype, or complex64 (m,); a longer tail is cut to them); halo_given / left_halo do
        not apply.  The pass's Costas exchange is recorded in `last_costas`; the result always carries the shard's qad.
        auto_center (the same on every rank: it adds collectives): a PSK pass calls `detect_center` on the demodulated signal once the
        Costas exchange has written it and builds its pulse table with the detected center (p.center where detection gives None);
        `last_center` is the value used.  ASK / FSK raise ValueError: their fused hot kernel needs the center before the demodulated
        signal exists.  The recipe there is two passes: one with want_qad=True, `detect_center(result.qad)`, then a second pass with
        that center -- or `iq_to_bits_auto(auto_center=True)`, which demodulates the shard once, detects the center across the shards and
        slices from the demodulated signal; it also takes auto_noise (every modulation).
        msg_records: refused (ValueError) as an option of the pass -- a message's middle window may lie in another rank's shard; the recipe is
        iq_to_bits, then `message_records` on the same shard and the pass's result.
        dc_correction: refused (ValueError) as an option of the pass; the recipe is `dc_correct` (the mean of the WHOLE capture, carried
        across the ranks), then iq_to_bits on the result -- with left_halo / left_raw corrected through its `also`."""
        e, c = self.engine, self.comm
        if dc_correction:
            raise ValueError("DC correction is not an option of a sharded pass: call dc_correct on the shard first, then iq_to_bits on the result")
        if msg_records:
            raise ValueError("message records are not an option of a sharded pass: call message_records(iq_local, result, p) after iq_to_bits")
        if auto_center and p.modulation_type != "PSK":
            raise ValueError("auto_center needs a PSK pass: for ASK / FSK run a pass with want_qad=True, detect_center(result.qad), "
                             "then a second pass with that center")
        _, pos_base, n_total = self._shard_range(iq_local, pos_base, n_total)
        if p.modulation_type == "PSK":
            return self._iq_to_bits_psk(iq_local, p, pos_base, n_total, left_raw, bool(auto_center))
        self.last_center = p.center
        left = self._left_halo(halo_given, left_halo)
        pending = None
        if not halo_given:
            # the halo exchange overlaps the hot kernel (all chunks but the first); on a pipelined engine it is issued on the tail
            # stream (behind the previous pass's exchanges), which first waits for whatever produced the shard on the caller's stream
            with (e.halo_context() if hasattr(e, "halo_context") else contextlib.nullcontext()):
                pending = c.all_gather_start(e.tail(iq_local, p))
            if hasattr(e, "runs_begin"):
                e.runs_begin(iq_local, pos_base, n_total, self.rank, self.world, p, want_qad)
        elif hasattr(e, "runs_launch"):            # the whole hot launch, on the hot stream
            e.runs_launch(iq_local, left, pos_base, n_total, self.rank, self.world, p, want_qad)
        # Everything after the hot kernel -- the wait for the halo, the first chunk, the all-gathers -- is issued on the engine's tail
        # stream when it is pipelined: the next pass's hot kernel then overlaps this pass's latency-bound tail, and the hot stream
        # never waits for a collective (the exchanges of one process group run in issue order: the halo of pass i + 1 sits behind the
        # last exchange of pass i's tail, so a hot stream that waited for its halo would run in lock-step with the tails).
        with (e.tail_context() if hasattr(e, "tail_context") else contextlib.nullcontext()):
            if pending is not None:
                halos = pending()
                left = halos[self.rank - 1] if self.rank > 0 else None
            return self._table_tail(iq_local, left, pos_base, n_total, p, want_qad)

    def iq_to_bits_auto(self, iq_local, p, auto_noise=False, auto_center=False, center_max_size=None, want_qad=True, pos_base=None, n_total=None,
                        halo_given=False, left_halo=None, left_raw=None):
        """The pass of DevicePipeline.iq_to_bits(auto_noise=..., auto_center=..., center_max_size=...) on a sharded capture, bit for bit: the
        same ShardResult as iq_to_bits (stitch, message_records, stitch_records and message_data work on it unchanged).  iq_local, pos_base,
        n_total, halo_given / left_halo, left_raw (PSK), want_qad: as iq_to_bits.
        auto_noise, auto_center and center_max_size MUST BE THE SAME ON EVERY RANK: they add collectives.
        auto_noise: noise = detect_noise_level(iq_local, pos_base, n_total) -- one all-gather, the same value on every rank -- and the pass
        runs with dataclasses.replace(p, noise_threshold=noise).  Where the noise level is not below the sample type's max_magnitude (compared
        as doubles) the reference demodulates nothing (Signal.py:474-484): EVERY rank raises ValueError, decided from the gathered value, and
        none enters a further collective.  What the reference raises for a level that is not a number (math.ceil) is raised on every rank alike.
        auto_center: the pulse table is built with detect_center(demodulated signal of the WHOLE capture, center_max_size); p.center where
        that gives None.  PSK: the PSK pass of iq_to_bits.  ASK / FSK: the shard is demodulated once into the result's qad together with the
        seam value (the demodulated value of the sample before the shard, from the two raw samples of the halo), the center is detected
        across the shards, and runs, rows and bits follow from the qad with that center (module docstring, "Automatic passes").  This route
        needs want_qad=True and an engine that is not pipelined (ValueError otherwise: it reads gathered values on the host).
        Without auto_center, ASK / FSK take the fused pass of iq_to_bits with the replaced parameters (a pipelined engine is fine there).
        Modulations other than ASK, FSK and PSK raise ValueError.  Everything a rank can get wrong on its own is refused before the first
        collective.  `last_center` is the center the pulse table was built with; `last_auto` = {"noise": the detected level or None,
        "center": the center used, "center_detected": whether detect_center found it, "all_gathers": all-gathers of this call}.  ASK / FSK
        with auto_center: the halo's unless halo_given, detect_center's, summaries + (ASK) merge + flags, one more with auto_noise."""
        import dataclasses
        from ..sniffer import max_magnitude
        e = self.engine
        auto_noise, auto_center = bool(auto_noise), bool(auto_center)
        mod = p.modulation_type
        if mod not in ("ASK", "FSK", "PSK"):
            raise ValueError(f"iq_to_bits_auto: ASK, FSK and PSK passes only (got {mod})")
        if auto_center and not want_qad:
            raise ValueError("auto_center needs the demodulated signal (want_qad=True)")
        if center_max_size is not None and int(center_max_size) < 0:
            raise ValueError("detect_center: max_size must not be negative")
        _, pos_base, n_total = self._shard_range(iq_local, pos_base, n_total, "iq_to_bits_auto")
        psk = mod == "PSK"
        own_route = auto_center and not psk
        # everything this rank can get wrong on its own, now: later refusals would leave the other ranks in a collective
        if auto_noise:
            self._estimator_engine("noise_partials")
        if psk or own_route:
            if n_total <= 2:
                raise ValueError(f"{mod}: a capture of two samples or fewer does not shard")
            if getattr(e, "tail_stream", None) is not None:
                raise ValueError(f"{'PSK shards run' if psk else 'an ASK / FSK pass with auto_center runs'} on an engine that is not pipelined: "
                                 "gathered values are read on the host between the phases")
        if psk:
            self._check_psk_own(p, pos_base, n_total, left_raw, auto_center)
        else:
            self._left_halo(halo_given, left_halo, view=False)
            if own_route:
                self._estimator_engine("demod_own", "demod", "demod_qad", "set_center", "compact_gt", "pairwise_partial", "histogram")
                e.demod_own(iq_local, left_halo if (halo_given and self.rank > 0) else None)
        with self._counting() as counted:
            noise = None
            if auto_noise:
                noise = self.detect_noise_level(iq_local, pos_base, n_total)       # raises on every rank alike (gathered statistics)
                dt = str(iq_local.dtype).replace("torch.", "")
                limit = max_magnitude(np.float32 if dt == "complex64" else dt)
                if not (float(noise) < float(limit)):                               # decided from the gathered value: every rank raises
                    raise ValueError(f"iq_to_bits_auto: the detected noise level {float(noise)!r} is not below the sample type's max_magnitude "
                                     f"{float(limit)!r}: the reference demodulates nothing of such a capture (Signal.quad_demod)")
                p = dataclasses.replace(p, noise_threshold=noise)
            self._center_found = False
            if psk:
                res = self._iq_to_bits_psk(iq_local, p, pos_base, n_total, left_raw, auto_center, center_max_size)
            elif not own_route:
                res = self.iq_to_bits(iq_local, p, want_qad=want_qad, pos_base=pos_base, n_total=n_total, halo_given=halo_given, left_halo=left_halo)
            else:
                res = self._iq_to_bits_demod_first(iq_local, p, pos_base, n_total, bool(halo_given), left_halo, center_max_size)
        self.last_auto = {"noise": noise, "center": self.last_center, "center_detected": self._center_found, "all_gathers": counted.count}
        return res

    def _iq_to_bits_demod_first(self, iq_local, p, pos_base, n_total, halo_given, left_halo, center_max_size):
        """ASK / FSK with auto_center (module docstring, "Automatic passes"); the caller has checked this rank's arguments"""
        e, c = self.engine, self.comm
        left = self._left_halo(halo_given, left_halo)
        if not halo_given:
            halos = c.all_gather(e.tail(iq_local, p))
            left = halos[self.rank - 1] if self.rank > 0 else None
        e.demod(iq_local, left, pos_base, n_total, self.rank, self.world, p)
        self.last_center = p.center
        center = self.detect_center(e.demod_qad(), center_max_size)
        if center is not None:
            self.last_center = float(center)
            self._center_found = True
            e.set_center(self.last_center)
        return self._table_tail(iq_local, left, pos_base, n_total, p, True)       # the runs from the qad; their left halo is the seam value

    def message_records(self, iq_local, result, p, message_length_divisor=1, pos_base=None, n_total=None):
        """One urhgpu_msg_record (protocol.RECORD_DTYPE) per message that closes on this rank, in order, as a numpy structured array: the
        ASK padding to message_length_divisor, the first and the middle bit's position and the RSSI (records.py).
        Called on EVERY rank after iq_to_bits with the shard that pass demodulated (after dc_correct: the corrected shard) and its result;
        pos_base / n_total default as in iq_to_bits.  The ranks' arrays concatenated in rank order are the records of
        DevicePipeline.iq_to_bits(msg_records=True, message_length_divisor=d) on the whole capture, RSSI bit patterns included.  ASK, FSK and
        PSK passes alike; only the padding depends on the modulation.
        Synchronous: gathered words are read on the host.  Two all-gathers, a third where a first message's window is not wholly inside its
        closing rank's shard, none on one rank; shards that do not tile [0, n_total) raise ValueError on every rank (decided from gathered
        data).  A rank that closes no message returns an empty array and takes part in every collective.  `last_records` records the number of
        all-gathers and of exchanged windows.  On a pipelined engine the device work runs behind the pass's tail."""
        e = self._estimator_engine("records_summary", "records_lookup", "records_window_part", "records_finish")
        if not p.write_bit_sample_pos:
            raise ValueError("message_records needs the positions of the pass (write_bit_sample_pos)")
        divisor = int(message_length_divisor)
        if divisor < 1 or divisor > 1 << 30:
            raise ValueError("message_records: 1 <= message_length_divisor <= 2^30")
        _, pos_base, n_total = self._shard_range(iq_local, pos_base, n_total)
        sps = int(p.samples_per_symbol)
        with self._counting() as c, (e.tail_context() if hasattr(e, "tail_context") else contextlib.nullcontext()):
            gather = c.all_gather if self.world > 1 else (lambda t: t[None])      # one rank: no collective
            words = gather(e.records_summary(iq_local, result, pos_base)).cpu().numpy()
            plan = records_plan(words, n_total, sps, divisor if p.modulation_type == "ASK" else 1)      # raises on every rank alike
            values = gather(e.records_lookup(result, records_requests(plan, self.rank))).cpu().numpy()
            firsts, outside = records_windows(plan, words, values, n_total, sps)
            window = None
            if outside:
                spans = [(firsts[r]["lo"], firsts[r]["w"]) for r in outside]
                parts = gather(e.records_window_part(iq_local, pos_base, spans, max(k for _, k in spans)))
                mine = firsts[self.rank]
                if mine is not None and mine["slot"] >= 0:
                    w = np.ascontiguousarray(np.asarray(words)).view(np.int64).reshape(self.world, REC_SUMMARY_WORDS)
                    lo, hi = mine["lo"], mine["lo"] + mine["w"]
                    window = parts.new_empty((mine["w"],) + tuple(parts.shape[3:]))           # contiguous, in the engine's memory
                    for q in range(self.world):                   # the shards tile the capture: every sample comes from exactly one rank
                        a, b = max(lo, int(w[q, REC_POS_BASE])), min(hi, int(w[q, REC_POS_BASE] + w[q, REC_N_LOCAL]))
                        if b > a:
                            window[a - lo:b - lo] = parts[q, mine["slot"], a - lo:b - lo]
            first = np.zeros(REC_FIRST_WORDS, np.int64)
            m, f = plan[self.rank], firsts[self.rank]
            if m is not None:
                first[:4] = (1, m["L"], m["np"], m["n_pad"])
                if f is not None:
                    first[4:] = (f["first_pos"], f["mid_pos"], 1, 1 if window is not None else 0)
            rec = e.records_finish(iq_local, result, pos_base, n_total, p, divisor, first, window)
        self.last_records = {"all_gathers": c.count, "windows": len(outside)}
        return rec

    def _iq_to_bits_psk(self, iq_local, p, pos_base, n_total, left_raw, auto_center=False, center_max_size=None):
        """the PSK pass (costas.py, steps 0-4).  Everything a rank can get wrong on its own is checked before the first collective."""
        e, c = self.engine, self.comm
        left_raw = self._check_psk_own(p, pos_base, n_total, left_raw, auto_center)
        summary = e.costas_spec(iq_local, left_raw, pos_base, n_total, self.rank, self.world, p)
        rounds = costas_exchange(c, summary, e.costas_resolve, e.costas_end)
        by_map, by_ckpt, serial, respec = e.costas_stats()
        self.last_costas = {"rounds": rounds, "chunks_by_map": by_map, "chunks_by_checkpoint": by_ckpt, "chunks_serial": serial,
                            "respeculation_rounds": respec}
        lasts = c.all_gather(e.costas_last())                 # every shard's last demodulated value: the seam of the pulse table
        left = lasts[self.rank - 1] if self.rank > 0 else None
        self.last_center = p.center
        if auto_center:
            center = self.detect_center(e.costas_qad(), center_max_size)
            if center is not None:
                self.last_center = float(center)
                self._center_found = True
                e.set_center(self.last_center)
        return self._table_tail(iq_local, left, pos_base, n_total, p, True)


def stitch(pieces):
    """Concatenate the per-rank pieces (rank order) of a sharded result into the single-GPU / reference
    shaped flat result.  pieces[r] = dict(rows, bits, msg_end, pauses, pos, pos_end) of numpy arrays, where
    msg_end / pos_end are LOCAL end offsets (in that rank's bits / pos) of the messages that close on rank r.
    Returns (ppseq, bits, msg_off, pauses, pos, pos_off)."""
    rows = np.concatenate([np.asarray(p["rows"], dtype=np.int64).reshape(-1, 2) for p in pieces])
    bits = np.concatenate([np.asarray(p["bits"], dtype=np.uint8) for p in pieces])
    pos = np.concatenate([np.asarray(p["pos"], dtype=np.int64) for p in pieces])
    pauses = np.concatenate([np.asarray(p["pauses"], dtype=np.int64) for p in pieces])
    msg_off, pos_off = [0], [0]
    b0 = p0 = 0
    for p in pieces:
        msg_off.extend((b0 + np.asarray(p["msg_end"], dtype=np.int64)).tolist())
        pos_off.extend((p0 + np.asarray(p["pos_end"], dtype=np.int64)).tolist())
        b0 += len(p["bits"])
        p0 += len(p["pos"])
    return rows, bits, np.array(msg_off, np.int64), pauses, pos, np.array(pos_off, np.int64)
