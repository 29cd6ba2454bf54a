// pass.hip -- the single-GPU pass (hot launch, pulse table, bits) and what every kind of pass shares with it (pass.hpp).
#include "pass.hpp"

namespace urh {

// Argument checks shared by every entry point that cuts a capture into chunks or turns rows into bits.  The reference
// takes `tolerance` as uint16 (OverflowError outside 0..65535, signal_functions.pyx:392) and divides by
// samples_per_symbol (ZeroDivisionError, ProtocolAnalyzer.py:353); here both are URHGPU_ERR_ARG before anything is launched.
int check_params(const urhgpu_params *p, bool need_sps) {
    if (p->tolerance < 0 || p->tolerance > 65535) return URHGPU_ERR_ARG;
    if (need_sps && (p->samples_per_symbol < 1 || p->bits_per_symbol < 1)) return URHGPU_ERR_ARG;
    return URHGPU_OK;
}

Plan make_plan(const urhgpu_ctx *ctx, int64_t n, int tol) {
    Plan pl;
    // whole tiles are grouped into chunks of tiles_per_chunk tiles (one workgroup each); a partial
    // tile at the end of the capture is one more chunk (see launch_runs_4 in demod_runs.hip)
    const int64_t full_tiles = n / kTile;
    const int64_t target = (int64_t)ctx->prop.multiProcessorCount * 16;      // chunks (four wavefronts each in the bit-plane kernel): ~2 rounds of the resident set
    // at most 4 tiles = 64 rows per chunk: the bit-plane kernel parks one row per lane (kBpMaxRows)
    int64_t tiles_per_chunk = std::min<int64_t>(4, std::max<int64_t>(1, (full_tiles + target - 1) / target));
    if (g_force_tiles_per_chunk >= 1 && g_force_tiles_per_chunk <= 4) tiles_per_chunk = g_force_tiles_per_chunk;
    pl.chunk_len = tiles_per_chunk * kTile;
    pl.n_chunks = (full_tiles * kTile + pl.chunk_len - 1) / pl.chunk_len + ((n % kTile) ? 1 : 0);
    pl.slab_stride = pl.chunk_len / ((int64_t)tol + 1) + 2;
    return pl;
}

size_t digitize_scratch_bytes(const Plan &pl, int64_t cap_rows, bool ask, bool bits) {
    size_t b = 0;
    b += align256((size_t)(pl.n_chunks + kMaxWorld) * sizeof(ChunkInfo));
    b += align256((size_t)pl.n_chunks * pl.slab_stride * 8);
    b += align256(resolve_scratch_bytes(pl.n_chunks + kMaxWorld)) + 2 * 256;
    b += align256(tile_tail_bytes(pl.n_chunks + kMaxWorld)) + 256;
    if (ask) b += align256((size_t)cap_rows * 16) + align256(merge_scratch_bytes(cap_rows));
    if (bits) b += align256(bits_scratch_bytes(cap_rows));
    b += 4096;
    return b;
}

static float noise_for(const urhgpu_params *p) {
    switch (p->mod) {
        case URHGPU_MOD_ASK: return 0.0f;
        case URHGPU_MOD_FSK:
        case URHGPU_MOD_PSK: return -4.0f;
        default: return p->noise_other;
    }
}

// reference: signal_functions.pyx:343-354 (double sqrt of the integer constant, stored to float)
static int max_magnitude_for(int dtype, float *out) {
    switch (dtype) {
        case URHGPU_DT_I8: *out = (float)sqrt(32513.0); return URHGPU_OK;
        case URHGPU_DT_U8: *out = (float)sqrt(65025.0); return URHGPU_OK;
        case URHGPU_DT_I16: *out = (float)sqrt(2147418113.0); return URHGPU_OK;
        case URHGPU_DT_U16: *out = (float)sqrt(4294836225.0); return URHGPU_OK;
        case URHGPU_DT_F32: *out = (float)sqrt(2.0); return URHGPU_OK;
        default: return URHGPU_ERR_DTYPE;
    }
}

// The pass-wide part of the hot kernel's arguments.  Left to the caller: in / qad / left_halo, chunks / slab, lds_pad (0), the launch range, and
// what only one kind of pass has (segment counters, seg_mode, the stream's own word on wide_int).  from_iq = false: the kernel reads an already
// demodulated signal -- no max_magnitude (and no dtype to get one from).
int hot_run_args(const urhgpu_ctx *ctx, const urhgpu_params *p, const Plan &pl, int64_t n, int64_t pos_base, bool from_iq, RunArgs *a) {
    if (p->bits_per_symbol < 1 || p->bits_per_symbol > 7) return URHGPU_ERR_UNSUPPORTED;
    memset(a, 0, sizeof(*a));
    a->order = 1 << p->bits_per_symbol;
    urhgpu_get_center_thresholds(p->center, p->center_spacing, a->order, a->thr);
    a->n = n; a->pos_base = pos_base;
    a->chunk_len = pl.chunk_len; a->slab_stride = pl.slab_stride;
    a->noise_sqrd = p->noise_threshold * p->noise_threshold;
    a->noise_val = noise_for(p);
    a->tol = p->tolerance;
    a->wide_int = ctx->tune_wide_int ? 1 : 0;                // (a one-shot pass has no probe of its capture to go by: the caller's word)
    return from_iq ? max_magnitude_for(p->dtype, &a->max_magnitude) : URHGPU_OK;
}

// One profile record = four events: [4k], [4k+1] bracket the hot launch on the stream (what is reported for launches made of
// several kernels); [4k+2], [4k+3] are attached to the bit-plane kernel's dispatch (its own begin / end timestamps)
static bool prof_begin_record(urhgpu_ctx *ctx, hipStream_t s, HotEvents *ev) {
    const bool prof = ctx->prof_on && (size_t)(4 * ctx->prof_used + 3) < ctx->prof_events.size();
    if (!prof) return false;
    // the stream-level bracket costs two more barrier packets around the hot launch (about 10 us of bubbles per pass): only
    // on request (URH_PROFILE_BRACKET, comparison of the two timings); the dispatch-attached pair costs nothing extra
    if (ctx->prof_bracket && hipEventRecord(ctx->prof_events[4 * ctx->prof_used], s) != hipSuccess) return false;
    ev->start = ctx->prof_events[4 * ctx->prof_used + 2];
    ev->stop = ctx->prof_events[4 * ctx->prof_used + 3];
    return true;
}
static int prof_end_record(urhgpu_ctx *ctx, hipStream_t s, bool used) {
    if (ctx->prof_bracket) URH_HIP(hipEventRecord(ctx->prof_events[4 * ctx->prof_used + 1], s));
    else if (!used) return URHGPU_OK;             // a launch made of several kernels (state-byte path): no record without the bracket
    if ((size_t)ctx->prof_used >= ctx->prof_dispatch.size()) ctx->prof_dispatch.resize((size_t)ctx->prof_used + 1);
    ctx->prof_dispatch[(size_t)ctx->prof_used] = used;
    ctx->prof_used += 1;
    return URHGPU_OK;
}

// The hot launch of a pass with its bookkeeping, on stream s: the profile record, the kernel, its completion event, the hand-over.
//   offer     the dispatch is offered `fallback` as its own completion signal (the profile record's stop event while one is open): an event
//             recorded behind the kernel is one more barrier packet between two hot kernels
//   fallback  recorded behind the launch where the dispatch took no event (not offered, or the state-byte kernel); nullptr: nobody waits (no s_tail)
//   s_tail    waits for the kernel; so does the caller's stream when s is the masked hot stream: what the caller queues on ITS stream afterwards
//             (overwriting the capture, the allocator handing its memory out again) must come behind the kernel.  (The NULL stream synchronises
//             with the masked stream by itself.)  nullptr: the caller queues the waits itself, on *hot_done.  A launch error drops the events.
int hot_launch(urhgpu_ctx *ctx, const RunArgs &a, const urhgpu_params *p, bool from_iq, hipStream_t s, bool offer, hipEvent_t fallback,
               hipStream_t s_tail, hipEvent_t *hot_done_out) {
    HotEvents ev;
    const bool prof = prof_begin_record(ctx, s, &ev);
    if (offer && !prof) ev.stop = fallback;
    URH_TRY(from_iq ? launch_demod_runs_iq(a, p->dtype, p->mod, a.qad != nullptr, s, &ev) : launch_runs_qad(a, s, &ev));
    hipEvent_t hot_done = (offer && ev.used) ? ev.stop : nullptr;
    if (prof) URH_TRY(prof_end_record(ctx, s, ev.used));
    if (fallback && !hot_done) { URH_HIP(hipEventRecord(fallback, s)); hot_done = fallback; }
    if (s_tail) {
        URH_HIP(hipStreamWaitEvent(s_tail, hot_done, 0));
        if (s != ctx->stream && ctx->stream != nullptr) URH_HIP(hipStreamWaitEvent(ctx->stream, hot_done, 0));
    }
    if (hot_done_out) *hot_done_out = hot_done;
    return URHGPU_OK;
}

// Every capture takes the CU-masked hot stream in pipelined mode.  Until round 5 integer captures kept the caller's stream --
// their kernel ALONE loses 2-5 % on 224 CUs (it is VALU-bound: profiles/r03a_mask_policy_probe.txt) --, but beside a hot kernel that
// fills all 256 CUs the previous pass's tail finds no wave slots and the passes serialise: pipelined steps through the capture stream
// 0.348 -> 0.280 ms (int16) and 0.361 -> 0.276 ms (int8) with the mask, complex64 unchanged (profiles/r05_dtype_stream_ab.txt).
// pipelined passes: the stream the hot kernel is launched on -- the CU-masked private one (see urhgpu_ctx_set_pipelined), ordered
// behind what the caller has queued on the context's stream so far
int hot_stream_begin(urhgpu_ctx *ctx, hipStream_t *out) {
    *out = ctx->stream;
    if (!ctx->pipelined || !ctx->hot_masked) return URHGPU_OK;
    hipStream_t hot = ctx->hot_masked;
    // The masked stream has default flags: what the caller has queued on the NULL stream is ordered before its work by the runtime
    // itself (and costs nothing when the NULL stream is idle).  An explicit event on the NULL stream would make THAT stream wait for the
    // previous hot kernel first and hand over afterwards: two cross-queue hand-overs between consecutive hot kernels (measured: a
    // 50 us gap instead of 5).  Any other stream of the caller's hands over through an event.
    if (ctx->stream != nullptr) {
        URH_HIP(hipEventRecord(ctx->ev_in, ctx->stream));
        URH_HIP(hipStreamWaitEvent(hot, ctx->ev_in, 0));
    }
    *out = hot;
    return URHGPU_OK;
}
// scratch (from the arena) and persistent descriptors of the tile tail over a table of n_entries chunks
int tile_tail_mem(urhgpu_ctx *ctx, int64_t n_entries, bool expands_bits, TileTailMem *tm) {
    tm->mem = ctx->arena.take(tile_tail_bytes(n_entries));
    tm->n_chunks = n_entries; tm->huge_count = ctx->d_tickets + 8;
    tm->parity = expands_bits ? (ctx->tile_parity ^= 1) : ctx->tile_parity;   // only passes that expand bits consume a counter
    tm->d_row_base = nullptr;
    if (!tm->mem) return URHGPU_ERR_ARG;
    URH_TRY(reserve_rdesc(ctx, n_entries));
    tm->rdesc = ctx->d_rdesc; tm->epoch = ++ctx->scan_epoch;
    return URHGPU_OK;
}
// look-back descriptors of the tile tail's resolve scan over a table of n_entries chunks: dedicated memory, zeroed when (re)allocated
int reserve_rdesc(urhgpu_ctx *ctx, int64_t n_entries) {
    const size_t rd = tile_rdesc_bytes(n_entries);
    if (rd > ctx->rdesc_cap) {
        if (ctx->d_rdesc) { URH_HIP(hipFree(ctx->d_rdesc)); ctx->d_rdesc = nullptr; ctx->rdesc_cap = 0; }
        const size_t want = (rd + 65535) & ~size_t(65535);
        URH_HIP(hipMalloc(&ctx->d_rdesc, want));
        URH_HIP(hipMemset(ctx->d_rdesc, 0, want));
        // (the memset is work of the NULL stream: it runs behind everything queued on the blocking streams -- a hot kernel that waits for
        // an upload --, and the tail's non-blocking streams do not wait for it: descriptors published by the pass's first kernels were
        // wiped by it.  Allocation time only: wait until it has happened.)
        center_note_wait();
        URH_HIP(hipDeviceSynchronize());
        ctx->rdesc_cap = want;
    }
    return URHGPU_OK;
}
// every allocation an auto-center pass over up to n_max samples would otherwise make when it first needs it (each one waits for the device):
// the center chain's scratch and the descriptor memory of the tail's scans.  Capture streams call it before their first push.
int reserve_auto_center_pass(urhgpu_ctx *ctx, int64_t n_max, int tolerance, int64_t cap_rows) {
    URH_TRY(reserve_center_chain(ctx, n_max));
    return reserve_pass_descriptors(ctx, n_max, tolerance, cap_rows);
}
// ... the descriptor memory alone (a stream of automatic-noise passes: the noise chain's scratch is part of the context)
int reserve_pass_descriptors(urhgpu_ctx *ctx, int64_t n_max, int tolerance, int64_t cap_rows) {
    const Plan pl = make_plan(ctx, n_max, tolerance);
    // chunks of a shorter capture: at most one per tile up to the plan's target, see make_plan
    const int64_t n_chunks = std::max<int64_t>(pl.n_chunks, (int64_t)ctx->prop.multiProcessorCount * 16 + 2);
    URH_TRY(reserve_rdesc(ctx, n_chunks));
    ScanState ss;
    return scan_state(ctx, tile_desc_cap(std::max<int64_t>(cap_rows, 1), n_chunks), &ss);
}

// resolve / emit arguments over the chunk table of a single-GPU pass: every chunk local, no summaries, the table's last row written here
void table_args(urhgpu_ctx *ctx, const urhgpu_params *p, const Plan &pl, int64_t n, ChunkInfo *chunks, uint64_t *slab, void *rs_mem, int64_t *rows,
                int64_t cap_rows, int64_t *d_n_acc, int64_t *d_n_rows, int64_t *d_n_rows_needed, bool ask, ResolveArgs *r, EmitArgs *e) {
    memset(r, 0, sizeof(*r));
    r->sc = resolve_scratch_carve(rs_mem, pl.n_chunks);
    r->chunks = chunks; r->n_chunks = pl.n_chunks; r->n_total = n; r->tol = p->tolerance;
    r->rows = rows; r->cap_rows = cap_rows; r->d_n_acc = d_n_acc; r->d_n_rows = d_n_rows; r->d_n_rows_needed = d_n_rows_needed; r->write_last_row = 1;
    r->local_pass = 0; r->aux = (ResolveAux *)(ctx->d_tickets + 4); r->summary_out = nullptr; r->chunk_first = 0; r->n_local = pl.n_chunks; r->d_ts_carry = nullptr;
    e->sc = r->sc;
    e->chunks = chunks; e->chunk_first = 0; e->slab = slab; e->slab_stride = pl.slab_stride;
    e->rows = rows; e->cap_rows = cap_rows; e->d_ts_carry = nullptr; e->is_ask = ask ? 1 : 0; e->sps = p->samples_per_symbol;
}

// Core of grab_pulse_lens / the fused path: run-segmentation kernel (IQ or qad source), resolve,
// emit rows, optional ASK merge.  On return d_rows / d_n_rows hold the final pulse table.
// scratch must come from ctx->arena (already reserved by the caller).
int digitize(urhgpu_ctx *ctx, bool from_iq, const void *d_in, int64_t n, const urhgpu_params *p, float *d_qad, int64_t *d_rows, int64_t cap_rows,
             int64_t *d_n_rows, int64_t *d_n_rows_needed, int64_t *d_n_acc, const Plan &pl, int seg_mode, hipStream_t s_tail, const BitsParams *tile_bp,
             TileTailMem *tile_out, const float *d_thr, const float *d_noise) {
    hipStream_t s = ctx->stream;
    if (s_tail && from_iq) URH_TRY(hot_stream_begin(ctx, &s));
    if (tile_out) tile_out->mem = nullptr;
    RunArgs a;
    URH_TRY(hot_run_args(ctx, p, pl, n, 0, from_iq, &a));
    a.in = d_in; a.qad = d_qad;
    if (d_thr) { if (from_iq) return URHGPU_ERR_ARG; a.d_thr = d_thr; }      // (thresholds in device memory: the qad-input kernels only)
    if (d_noise) {                                           // (the noise threshold in device memory: the IQ-input kernels only, never the segmentation)
        if (!from_iq || seg_mode) return URHGPU_ERR_ARG;
        a.d_noise = d_noise;
        if (ctx->wide_int_auto) a.wide_int = 1;              // (what a capture stream's probe saw in the captures before)
    }
    a.lds_pad = ctx->pipelined ? ctx->hot_lds_pad : 0;
    if (seg_mode) {
        // message segmentation: state = (|sample| > noise threshold) with the 10-sample outlier tolerance.  Reuses the
        // ASK arithmetic with max_magnitude 1 (q = sqrtf(I*I + Q*Q) exactly), no noise gating, threshold = noise level.
        a.seg_mode = 1; a.max_magnitude = 1.0f; a.noise_sqrd = -1.0f; a.noise_val = __builtin_nanf("");
        if (d_qad) {
            // the pass also leaves afp_demod(iq, noise_threshold, "ASK") in d_qad (float32 captures; p->center is the noise threshold here)
            if (!from_iq || p->dtype != URHGPU_DT_F32) return URHGPU_ERR_UNSUPPORTED;
            a.dm_noise_sqrd = p->center * p->center; a.dm_noise_val = 0.0f;
            URH_TRY(max_magnitude_for(p->dtype, &a.dm_max_magnitude));
        }
    }
    ChunkInfo *chunks = (ChunkInfo *)ctx->arena.take((size_t)pl.n_chunks * sizeof(ChunkInfo));
    uint64_t *slab = (uint64_t *)ctx->arena.take((size_t)pl.n_chunks * pl.slab_stride * 8);
    if (!chunks || !slab) return URHGPU_ERR_ARG;
    a.chunks = chunks; a.slab = slab;
    // pipelined: the tail stream waits for the completion signal of the hot dispatch itself where one launch covers the capture (no
    // partial tile at the end); everything after the hot kernel goes to the tail stream
    URH_TRY(hot_launch(ctx, a, p, from_iq, s, s_tail && from_iq && n % kTile == 0, s_tail ? ctx->ev_hot : nullptr, s_tail, nullptr));
    if (s_tail) s = s_tail;

    const bool ask = (p->mod == URHGPU_MOD_ASK) && !seg_mode;
    int64_t *rows_stage = d_rows;
    int64_t *d_n_stage = d_n_rows;
    void *merge_scratch = nullptr;
    if (ask) {
        rows_stage = (int64_t *)ctx->arena.take((size_t)cap_rows * 16);
        merge_scratch = ctx->arena.take(merge_scratch_bytes(cap_rows));
        d_n_stage = (int64_t *)ctx->arena.take(64);
        if (!rows_stage || !merge_scratch || !d_n_stage) return URHGPU_ERR_ARG;
    }
    void *rs_mem = ctx->arena.take(resolve_scratch_bytes(pl.n_chunks));
    if (!rs_mem) return URHGPU_ERR_ARG;
    ResolveArgs r;
    EmitArgs e;
    table_args(ctx, p, pl, n, chunks, slab, rs_mem, rows_stage, cap_rows, d_n_acc, d_n_stage, d_n_rows_needed, ask, &r, &e);
    if (!ask && g_tile_tail) {
        // tile tail: one composed scan instead of three, rows + their bit aggregates in one pass (pulse_table.hip)
        TileTailMem tm;
        URH_TRY(tile_tail_mem(ctx, pl.n_chunks, tile_out != nullptr, &tm));
        URH_TRY(launch_tile_rows(r, e, tm, tile_out ? tile_bp : nullptr, s));
        if (tile_out) *tile_out = tm;
        URH_HIP(hipGetLastError());
        return URHGPU_OK;
    }
    URH_TRY(launch_resolve_emit_single(r, e, s));
    if (ask) URH_TRY(launch_merge_rows_ask(rows_stage, d_n_stage, cap_rows, d_rows, cap_rows, d_n_rows, merge_scratch, ctx->d_tickets, s));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

BitsParams bits_params(const urhgpu_params *p) {
    BitsParams bp;
    bp.sps = (int64_t)p->samples_per_symbol;
    bp.bps = p->bits_per_symbol;
    bp.pause_threshold = p->pause_threshold;
    bp.samples_per_bit = (int64_t)((double)p->samples_per_symbol / (double)p->bits_per_symbol);   // int(sps / bps) :344
    bp.write_pos = p->write_bit_sample_pos ? 1 : 0;
    bp.d_row_base = nullptr; bp.d_ts_carry = nullptr; bp.d_absorbed = nullptr; bp.d_extra = nullptr; bp.is_last_rank = 1;
    bp.d_rows_needed = nullptr;
    return bp;
}

// descriptor memory of the single-pass scans for pulse tables of up to cap_rows rows
int scan_state(urhgpu_ctx *ctx, int64_t cap_rows, ScanState *out) {
    const size_t need = bits_desc_bytes(cap_rows);
    if (need > ctx->desc_cap) {
        if (ctx->d_desc) { URH_HIP(hipFree(ctx->d_desc)); ctx->d_desc = nullptr; ctx->desc_cap = 0; }
        const size_t want = (need + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1);
        URH_HIP(hipMalloc(&ctx->d_desc, want));
        URH_HIP(hipMemset(ctx->d_desc, 0, want));
        center_note_wait();
        URH_HIP(hipDeviceSynchronize());                   // (see tile_tail_mem: the NULL stream's memset must not land behind the pass's kernels)
        ctx->desc_cap = want;
    }
    out->tickets = ctx->d_tickets; out->desc = ctx->d_desc; out->desc_bytes = ctx->desc_cap; out->epoch = &ctx->scan_epoch;
    return URHGPU_OK;
}

// pipelined mode: rotate to the scratch arena used three passes ago; the caller's stream first waits for the tail that used it.
// (Two arenas made the hot kernel of pass i + 2 wait for the tail of pass i -- whose row kernel, starved of wave slots by the hot kernel
// of pass i + 1, only finishes right after it: the passes ran back to back again.  With three the hot kernels follow each other and
// the tails trail one pass behind.)
int begin_pipelined_pass(urhgpu_ctx *ctx) {
    std::swap(ctx->arena, ctx->arena_alt);
    std::swap(ctx->arena_alt, ctx->arena_alt2);
    ctx->passes_begun += 1;
    // Has the tail that last used this arena finished?  A caller that runs more than two passes ahead of the GPU (a tight loop of
    // passes) is held back HERE, on the host, until it has (bounded run-ahead; the GPU still has the previous hot kernel queued
    // behind the running one): a stream-level wait would put one more barrier packet between two hot kernels (about 4 us of the
    // gap; measured in round 2, tools/ab.sh history in profiles/HISTORY.md).
    const hipError_t q = hipEventQuery(ctx->ev_tail[ctx->flip]);
    if (q == hipErrorNotReady) {
        (void)hipGetLastError();                   // "not ready" is an answer, not an error: keep it out of the sticky last-error slot
        center_note_wait();
        URH_HIP(hipEventSynchronize(ctx->ev_tail[ctx->flip]));
    } else if (q != hipSuccess) {
        URH_HIP(q);
    }
    return URHGPU_OK;
}
int end_pipelined_pass(urhgpu_ctx *ctx) {
    URH_HIP(hipEventRecord(ctx->ev_tail[ctx->flip], ctx->tail_stream));
    ctx->flip = (ctx->flip + 1) % 3;
    ctx->tail_pending = true;
    return URHGPU_OK;
}

int reserve_psk_pass(urhgpu_ctx *ctx, int64_t n_max, int tolerance, bool want_qad) {
    URH_TRY(ctx->aux.reserve(costas_scratch_bytes(n_max) + 1024));
    const Plan pl = make_plan(ctx, n_max, tolerance);
    // (as urhgpu_ctx_reserve sizes them: the densest pulse table there can be)
    const size_t bytes = digitize_scratch_bytes(pl, n_max / ((int64_t)tolerance + 1) + 2, true, true) + (want_qad ? 0 : align256((size_t)n_max * 4));
    URH_TRY(ctx->arena.reserve(bytes));
    URH_TRY(ctx->arena_alt.reserve(bytes));
    URH_TRY(ctx->arena_alt2.reserve(bytes));
    return URHGPU_OK;
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_get_center_thresholds(float center, float spacing, int modulation_order, float *out) {
    // signal_functions.pyx:380-390; int -> float conversion, fp32 multiply and add/sub, no contraction
    const int n = modulation_order / 2;
    for (int i = 0; i < n; ++i) out[i] = center - (float)(n - (i + 1)) * spacing;
    for (int i = n; i < modulation_order - 1; ++i) out[i] = center + (float)(i + 1 - n) * spacing;
    return URHGPU_OK;
}

// The Costas loop of a PSK pass on the context's stream, its scratch from ctx->aux.  Every Costas kernel of a context runs on that one
// stream, in order, so the one scratch serves passes that overlap further down (a pipelined pass's tail only reads the demodulated signal).
// (A capture longer than any before lets the arena grow: hipFree waits for the device first.  Capture streams reserve for n_max up front.)
static int costas_demod(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad, const float *d_noise = nullptr) {
    URH_TRY(ctx->aux.reserve(costas_scratch_bytes(n) + 1024));
    ctx->aux.reset();
    void *scratch = ctx->aux.take(costas_scratch_bytes(n));
    URH_TRY(launch_costas(ctx, d_iq, n, p, d_qad, scratch, d_noise));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// ---- device-pointer entry points -------------------------------------------------------------------
// afp_demod on the context's stream as it is: no wait for an earlier pass's tail (the demodulation takes no scratch from the pass arenas)
// d_noise: not nullptr -- the kernels gate with the noise_sqrd in THIS device float (a pass whose threshold was decided on the device)
static int afp_demod_queue(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad, const float *d_noise = nullptr) {
    if (n <= 2) {                                   // signal_functions.pyx:335-336
        if (n > 0) URH_HIP(hipMemsetAsync(d_qad, 0, (size_t)n * 4, ctx->stream));
        return URHGPU_OK;
    }
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)d_qad & 7)) return URHGPU_ERR_ARG;
    if (p->mod == URHGPU_MOD_PSK) return costas_demod(ctx, d_iq, n, p, d_qad, d_noise);
    RunArgs a;
    memset(&a, 0, sizeof(a));
    a.in = d_iq; a.qad = d_qad; a.n = n; a.left_halo = nullptr; a.d_noise = d_noise;
    a.noise_sqrd = p->noise_threshold * p->noise_threshold;
    a.noise_val = noise_for(p);
    URH_TRY(max_magnitude_for(p->dtype, &a.max_magnitude));
    const int64_t rows = (n + 511) / 512;                        // k_afp_demod: 512 samples per workgroup-wide load
    const int grid = (int)std::min<int64_t>(rows, (int64_t)ctx->prop.multiProcessorCount * 16);
    URH_TRY(launch_afp_demod(a, p->dtype, p->mod, grid, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_afp_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad) {
    if (!ctx || !p || n < 0 || (n > 0 && (!d_iq || !d_qad))) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    return afp_demod_queue(ctx, d_iq, n, p, d_qad);
}

int urhgpu_grab_pulse_lens_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t n, const urhgpu_params *p,
                               int64_t *d_rows, int64_t cap_rows, int64_t *d_n_rows) {
    if (!ctx || !p || n < 0 || cap_rows < 0 || !d_n_rows) return URHGPU_ERR_ARG;
    URH_TRY(check_params(p, false));
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    if (n == 0) {                                   // signal_functions.pyx:416-417
        URH_HIP(hipMemsetAsync(d_n_rows, 0, 8, ctx->stream));
        URH_HIP(hipMemsetAsync(ctx->d_counts, 0, 16 * 8, ctx->stream));
        return URHGPU_OK;
    }
    if (!d_qad || !d_rows || ((uintptr_t)d_qad & 7)) return URHGPU_ERR_ARG;
    const Plan pl = make_plan(ctx, n, p->tolerance);
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, cap_rows, p->mod == URHGPU_MOD_ASK, false)));
    ctx->arena.reset();
    return digitize(ctx, false, d_qad, n, p, nullptr, d_rows, cap_rows, d_n_rows, ctx->d_counts + 8, ctx->d_counts + 9, pl);
}

static int ppseq_to_bits_inner(urhgpu_ctx *ctx, const int64_t *d_rows, const int64_t *d_n_rows, int64_t cap,
                               const urhgpu_params *p, const urhgpu_outputs *out, void *scratch,
                               const int64_t *d_rows_needed = nullptr) {
    BitsOut bo{out->bits, out->cap_bits, out->msg_off, out->pauses, out->cap_msg, out->pos, out->cap_pos, out->pos_off, out->counts, out->h_counts};
    BitsParams bp = bits_params(p);
    bp.d_rows_needed = d_rows_needed;
    ScanState ss;
    URH_TRY(scan_state(ctx, cap, &ss));
    URH_TRY(launch_ppseq_to_bits(d_rows, d_n_rows, cap, bp, bo, scratch, ss, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_ppseq_to_bits_dev(urhgpu_ctx *ctx, const int64_t *d_rows, const int64_t *d_n_rows, int64_t cap_rows_hint,
                             const urhgpu_params *p, const urhgpu_outputs *out) {
    if (!ctx || !p || !out || !d_n_rows || cap_rows_hint < 0) return URHGPU_ERR_ARG;
    if (p->bits_per_symbol < 1 || p->samples_per_symbol < 1) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    const int64_t cap = std::max<int64_t>(cap_rows_hint, 1);
    URH_TRY(ctx->arena.reserve(bits_scratch_bytes(cap) + 4096));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(bits_scratch_bytes(cap));
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(ppseq_to_bits_inner(ctx, d_rows, d_n_rows, cap, p, out, scratch));
    if (out->blob) {                                       // compact mirror: out->rows must then be the table d_rows (and cap_rows its capacity)
        if (out->rows != d_rows) return URHGPU_ERR_ARG;
        URH_TRY(launch_pack_blob(out, p->write_bit_sample_pos, ctx->stream));
    }
    return URHGPU_OK;
}

// The automatic noise threshold of a pass (urhgpu_iq_to_bits_auto_dev): where its result block goes.  queue() puts the chain -- chunk
// statistics, k_noise_decide -- on the caller's stream, in front of whatever gates; the kernels then load block->noise_sqrd.
struct NoiseAuto {
    void *d_res, *h_res;
    const float *d_noise() const { return &((const urhgpu_noise_result *)d_res)->noise_sqrd; }
    int queue(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p) const {
        return launch_noise_chain(d_iq, p->dtype, n, urhgpu_noise_max_magnitude(p->dtype), p->noise_threshold, 1, ctx->d_noise_work, d_res, h_res, ctx->stream);
    }
};

static int iq_to_bits_impl(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out, const NoiseAuto *na) {
    if (!ctx || !p || !out || n <= 0 || !d_iq || !out->rows || !out->counts) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_TRY(check_params(p, out->bits != nullptr));
    if (((uintptr_t)d_iq & 15) || (out->qad && ((uintptr_t)out->qad & 7))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    const float *d_noise = na ? na->d_noise() : nullptr;
    if (na) URH_TRY(na->queue(ctx, d_iq, n, p));             // (its scratch is the context's own: no arena, no wait)
    const Plan pl = make_plan(ctx, n, p->tolerance);
    const bool ask = (p->mod == URHGPU_MOD_ASK);
    const bool fused = !(n <= 2 || p->mod == URHGPU_MOD_PSK);
    // a PSK pass on a pipelined context: the Costas kernels on the caller's stream (the device drives their rounds: the host never waits),
    // everything behind them -- segmentation of the demodulated signal, bits, pack -- on the tail stream, the arenas rotating as for fused passes
    const bool psk_piped = ctx->pipelined && ctx->tail_stream && p->mod == URHGPU_MOD_PSK && n > 2;
    const bool piped = ctx->pipelined && (fused || psk_piped);
    if (piped) URH_TRY(begin_pipelined_pass(ctx)); else URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, out->cap_rows, ask, true) + (out->qad ? 0 : align256((size_t)n * 4))));
    ctx->arena.reset();
    int64_t *d_n_rows = ctx->d_counts + 10;
    const bool want_bits = out->bits && out->msg_off && out->pauses && out->pos_off;
    BitsParams tile_bp = bits_params(p);
    tile_bp.d_rows_needed = ctx->d_counts + 8;
    TileTailMem tile;
    tile.mem = nullptr;
    if (!fused) {
        // no fused kernel: demodulate (zeros for n <= 2, Costas loop for PSK), then segment the qad
        float *qad = out->qad;
        if (!qad) { qad = (float *)ctx->arena.take((size_t)n * 4); if (!qad) return URHGPU_ERR_ARG; }      // (piped: the rotating arena's, not a later pass's)
        hipStream_t caller = ctx->stream;
        if (psk_piped) {
            URH_TRY(costas_demod(ctx, d_iq, n, p, qad, d_noise));
            URH_HIP(hipEventRecord(ctx->ev_hot, ctx->stream));
            URH_HIP(hipStreamWaitEvent(ctx->tail_stream, ctx->ev_hot, 0));
            ctx->stream = ctx->tail_stream;
        } else if (d_noise) {
            URH_TRY(afp_demod_queue(ctx, d_iq, n, p, qad, d_noise));
        } else {
            URH_TRY(urhgpu_afp_demod_dev(ctx, d_iq, n, p, qad));
        }
        const int sd = digitize(ctx, false, qad, n, p, nullptr, out->rows, out->cap_rows, d_n_rows, ctx->d_counts + 8,
                                ctx->d_counts + 9, pl, 0, nullptr, want_bits ? &tile_bp : nullptr, want_bits ? &tile : nullptr);
        ctx->stream = caller;
        URH_TRY(sd);
    } else {
        URH_TRY(digitize(ctx, true, d_iq, n, p, out->qad, out->rows, out->cap_rows, d_n_rows, ctx->d_counts + 8,
                         ctx->d_counts + 9, pl, 0, piped ? ctx->tail_stream : nullptr, want_bits ? &tile_bp : nullptr,
                         want_bits ? &tile : nullptr, nullptr, d_noise));
    }
    int st = URHGPU_OK;
    if (want_bits) {                                                         // else: pulse table only
        const int64_t cap = std::max<int64_t>(out->cap_rows, 1);
        void *scratch = ctx->arena.take(bits_scratch_bytes(cap));
        if (!scratch) return URHGPU_ERR_ARG;
        hipStream_t caller = ctx->stream;
        if (piped) ctx->stream = ctx->tail_stream;
        if (tile.mem) {
            BitsOut bo{out->bits, out->cap_bits, out->msg_off, out->pauses, out->cap_msg, out->pos, out->cap_pos, out->pos_off, out->counts, out->h_counts};
            ScanState ss;
            st = scan_state(ctx, tile_desc_cap(cap, pl.n_chunks), &ss);
            if (st == URHGPU_OK) st = launch_tile_bits(tile, out->rows, d_n_rows, cap, tile_bp, bo, scratch, ss, ctx->stream);
            if (st == URHGPU_OK && hipGetLastError() != hipSuccess) st = URHGPU_ERR_HIP;
        } else {
            st = ppseq_to_bits_inner(ctx, out->rows, d_n_rows, cap, p, out, scratch, ctx->d_counts + 8);
        }
        if (st == URHGPU_OK && out->blob) st = launch_pack_blob(out, p->write_bit_sample_pos, ctx->stream);     // compact mirror (compact.hip)
        ctx->stream = caller;
    } else if (out->blob) {
        st = URHGPU_ERR_ARG;                               // the blob mirrors the bit outputs: all of them must be given
    }
    ctx->last_tail = piped ? ctx->tail_stream : ctx->stream;
    if (piped) URH_TRY(end_pipelined_pass(ctx));
    return st;
}

int urhgpu_iq_to_bits_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p,
                          const urhgpu_outputs *out) {
    return iq_to_bits_impl(ctx, d_iq, n, p, out, nullptr);
}

// ---- automatic center inside a pass ------------------------------------------------------------------------------------------
// Every center chain of a context runs on ONE stream, in order -- the tail stream of a pipelined context, the caller's otherwise --, so the one
// scratch (ctx->center_work) serves passes that overlap further down.
static hipStream_t center_stream(urhgpu_ctx *ctx) { return (ctx->pipelined && ctx->tail_stream) ? ctx->tail_stream : ctx->stream; }

int urhgpu_detect_center_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t n, int64_t max_size, void *d_result, int64_t hist_cap) {
    if (!ctx || n < 0 || (n > 0 && !d_qad) || !d_result || hist_cap < 0) return URHGPU_ERR_ARG;
    CenterScope scope;                                       // (host waits below here are counted: urhgpu_test_center_host_syncs)
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = center_stream(ctx);
    if (s != ctx->stream) {                                  // the signal is the caller's stream's work: hand over, by events
        if (!ctx->ev_center) URH_HIP(hipEventCreateWithFlags(&ctx->ev_center, hipEventDisableTiming));
        URH_HIP(hipEventRecord(ctx->ev_center, ctx->stream));
        URH_HIP(hipStreamWaitEvent(s, ctx->ev_center, 0));
    }
    CenterChain c;
    URH_TRY(center_chain_async(ctx, d_qad, n, max_size, s, &c));
    URH_TRY(center_publish(c, nullptr, d_result, nullptr, hist_cap, s));
    if (s != ctx->stream) {                                  // ... and back: what the caller queues next sees the result
        URH_HIP(hipEventRecord(ctx->ev_center, s));
        URH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_center, 0));
    }
    return URHGPU_OK;
}

// The !fused shape of urhgpu_iq_to_bits_dev for every modulation: demodulate into out->qad, find the center of the demodulated signal, slice with
// it.  Nothing here waits for the device or reads anything back; on a pipelined context everything behind the demodulation goes to the tail stream.
static int iq_to_bits_auto_center_impl(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, int64_t max_size, const urhgpu_outputs *out,
                                       void *d_result, void *h_result, int64_t hist_cap, const NoiseAuto *na) {
    if (!ctx) return URHGPU_ERR_ARG;
    if (!p || !out || n <= 0 || !d_iq || !out->rows || !out->counts || !out->qad || !d_result || hist_cap < 0) return URHGPU_ERR_ARG;
    const bool want_bits = out->bits && out->msg_off && out->pauses && out->pos_off;
    if (!want_bits && out->blob) return URHGPU_ERR_ARG;      // the blob mirrors the bit outputs: all of them must be given
    CenterScope scope;                                       // (host waits below here are counted: urhgpu_test_center_host_syncs)
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_TRY(check_params(p, out->bits != nullptr));
    if (p->bits_per_symbol < 1 || p->bits_per_symbol > 7) return URHGPU_ERR_UNSUPPORTED;
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)out->qad & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    const float *d_noise = na ? na->d_noise() : nullptr;
    if (na) URH_TRY(na->queue(ctx, d_iq, n, p));             // (the noise chain: on the caller's stream, in front of the demodulation)
    const Plan pl = make_plan(ctx, n, p->tolerance);
    const bool ask = (p->mod == URHGPU_MOD_ASK);
    const bool piped = ctx->pipelined && ctx->tail_stream;
    if (piped) URH_TRY(begin_pipelined_pass(ctx)); else URH_TRY(join_tail(ctx));
    int64_t *d_n_rows = ctx->d_counts + 10;
    BitsParams tile_bp = bits_params(p);
    tile_bp.d_rows_needed = ctx->d_counts + 8;
    TileTailMem tile;
    tile.mem = nullptr;
    hipStream_t caller = ctx->stream;
    // from here on an error ends the pass like a success does: the arenas have rotated (begin_pipelined_pass), so ev_tail / flip must follow
    auto rest = [&]() -> int {
        URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, out->cap_rows, ask, true)));
        ctx->arena.reset();
        // the demodulation on the caller's stream (PSK: the Costas loop, its scratch from ctx->aux)
        if (p->mod == URHGPU_MOD_PSK && n > 2) URH_TRY(costas_demod(ctx, d_iq, n, p, out->qad, d_noise));
        else URH_TRY(afp_demod_queue(ctx, d_iq, n, p, out->qad, d_noise));
        if (piped) {
            URH_HIP(hipEventRecord(ctx->ev_hot, ctx->stream));
            URH_HIP(hipStreamWaitEvent(ctx->tail_stream, ctx->ev_hot, 0));
            ctx->stream = ctx->tail_stream;
        }
        CenterChain c;
        URH_TRY(center_chain_async(ctx, out->qad, n, max_size, ctx->stream, &c));
        URH_TRY(center_publish(c, p, d_result, h_result, hist_cap, ctx->stream));
        URH_TRY(digitize(ctx, false, out->qad, n, p, nullptr, out->rows, out->cap_rows, d_n_rows, ctx->d_counts + 8, ctx->d_counts + 9, pl, 0, nullptr,
                         want_bits ? &tile_bp : nullptr, want_bits ? &tile : nullptr, c.d_thr));
        if (!want_bits) return URHGPU_OK;                    // pulse table only
        const int64_t cap = std::max<int64_t>(out->cap_rows, 1);
        void *scratch = ctx->arena.take(bits_scratch_bytes(cap));
        if (!scratch) return URHGPU_ERR_ARG;
        if (tile.mem) {
            BitsOut bo{out->bits, out->cap_bits, out->msg_off, out->pauses, out->cap_msg, out->pos, out->cap_pos, out->pos_off, out->counts, out->h_counts};
            ScanState ss;
            URH_TRY(scan_state(ctx, tile_desc_cap(cap, pl.n_chunks), &ss));
            URH_TRY(launch_tile_bits(tile, out->rows, d_n_rows, cap, tile_bp, bo, scratch, ss, ctx->stream));
            URH_HIP(hipGetLastError());
        } else {
            URH_TRY(ppseq_to_bits_inner(ctx, out->rows, d_n_rows, cap, p, out, scratch, ctx->d_counts + 8));
        }
        if (out->blob) URH_TRY(launch_pack_blob(out, p->write_bit_sample_pos, ctx->stream));
        return URHGPU_OK;
    };
    const int st = rest();
    ctx->stream = caller;
    ctx->last_tail = piped ? ctx->tail_stream : ctx->stream;
    if (piped) URH_TRY(end_pipelined_pass(ctx));
    return st;
}

int urhgpu_iq_to_bits_auto_center_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, int64_t max_size, const urhgpu_outputs *out,
                                      void *d_result, void *h_result, int64_t hist_cap) {
    return iq_to_bits_auto_center_impl(ctx, d_iq, n, p, max_size, out, d_result, h_result, hist_cap, nullptr);
}

// ---- automatic noise threshold inside a pass ----------------------------------------------------------------------------------
// Signal.max_magnitude (Signal.py:404-406): (2 * max(min^2, max^2)) ** 0.5 over IQArray.min_max_for_dtype's bounds
double urhgpu_noise_max_magnitude(int dtype) {
    switch (dtype) {
        case URHGPU_DT_I8: return sqrt(2.0 * 128.0 * 128.0);
        case URHGPU_DT_U8: return sqrt(2.0 * 255.0 * 255.0);
        case URHGPU_DT_I16: return sqrt(2.0 * 32768.0 * 32768.0);
        case URHGPU_DT_U16: return sqrt(2.0 * 65535.0 * 65535.0);
        case URHGPU_DT_F32: return sqrt(2.0);
        default: return 0.0;
    }
}

int urhgpu_detect_noise_level_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, void *d_result) {
    if (!ctx || n < 0 || (n > 0 && !d_iq) || !d_result || ((uintptr_t)d_result & 7)) return URHGPU_ERR_ARG;
    if (dtype_bytes(dtype) == 0) return URHGPU_ERR_DTYPE;
    if ((uintptr_t)d_iq & (uintptr_t)(dtype_bytes(dtype) - 1)) return URHGPU_ERR_ARG;
    NoiseScope scope;                                        // (host waits below here are counted: urhgpu_test_noise_host_syncs)
    URH_HIP(hipSetDevice(ctx->device));
    return launch_noise_chain(d_iq, dtype, n, urhgpu_noise_max_magnitude(dtype), 0.0f, 0, ctx->d_noise_work, d_result, nullptr, ctx->stream);
}

int urhgpu_iq_to_bits_auto_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, int auto_noise, int auto_center,
                               int64_t center_max_size, const urhgpu_outputs *out, void *d_noise_result, void *h_noise_result,
                               void *d_center_result, void *h_center_result, int64_t hist_cap) {
    if (!ctx) return URHGPU_ERR_ARG;
    if (auto_center && (!out || !out->qad)) return URHGPU_ERR_ARG;       // the center is detected on the materialised demodulated signal
    if (!auto_noise) {
        if (auto_center) return urhgpu_iq_to_bits_auto_center_dev(ctx, d_iq, n, p, center_max_size, out, d_center_result, h_center_result, hist_cap);
        return urhgpu_iq_to_bits_dev(ctx, d_iq, n, p, out);
    }
    if (!d_noise_result || ((uintptr_t)d_noise_result & 7) || ((uintptr_t)h_noise_result & 7)) return URHGPU_ERR_ARG;
    NoiseScope scope;                                        // (host waits below here are counted: urhgpu_test_noise_host_syncs)
    const NoiseAuto na{d_noise_result, h_noise_result};
    if (auto_center) return iq_to_bits_auto_center_impl(ctx, d_iq, n, p, center_max_size, out, d_center_result, h_center_result, hist_cap, &na);
    return iq_to_bits_impl(ctx, d_iq, n, p, out, &na);
}

int64_t urhgpu_test_noise_host_syncs(void) { return (int64_t)urh::g_noise_host_syncs.load(); }

int64_t urhgpu_center_hist_cap(urhgpu_ctx *ctx) { return ctx ? (int64_t)ctx->tune_center_max_bins : 0; }

int64_t urhgpu_test_center_host_syncs(void) { return (int64_t)urh::g_center_host_syncs.load(); }

// The results of a pass that is over (out: the descriptor the pass was given, with out->blob / cap_blob naming a device blob), on the
// host: pack kernel, the header, then ONE copy of header.total_bytes -- what the boundary objects (Signal.bits(), BitsResult.ppseq() ...)
// fetch instead of the wide int64 tables.  host_dst: pinned memory (hipHostMalloc / torch pin_memory) for an asynchronous copy at PCIe
// speed; pageable memory works (the runtime stages it).  Synchronous.
int urhgpu_outputs_to_host(urhgpu_ctx *ctx, const urhgpu_outputs *out, int write_pos, void *host_dst, int64_t cap_dst, int64_t *total_bytes) {
    if (!ctx || !out || !out->blob || !host_dst || !total_bytes || cap_dst < URHGPU_BLOB_HEADER_BYTES) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_pack_blob(out, write_pos, ctx->stream));
    URH_HIP(hipGetLastError());
    int64_t *hdr = ctx->h_small ? (int64_t *)ctx->h_small : (int64_t *)host_dst;
    URH_HIP(hipMemcpyAsync(hdr, out->blob, URHGPU_BLOB_HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(wait_stream(ctx, ctx->stream));
    if (hdr[0] != URHGPU_BLOB_MAGIC) return URHGPU_ERR_ARG;
    const int64_t total = hdr[6] < 0 ? -hdr[6] : hdr[6];
    *total_bytes = total;
    if (hdr[6] < 0 || total > cap_dst) return URHGPU_ERR_CAPACITY;
    URH_HIP(hipMemcpyAsync(host_dst, out->blob, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

int64_t urhgpu_blob_capacity(int64_t cap_rows, int64_t cap_bits, int64_t cap_msg, int64_t cap_pos, int has_pos) {
    if (cap_rows < 0 || cap_bits < 0 || cap_msg < 0 || cap_pos < 0) return 0;
    return urh::blob_capacity(cap_rows, cap_bits, cap_msg, cap_pos, has_pos ? 1 : 0);
}

}  // extern "C"
