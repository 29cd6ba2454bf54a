// stream_pass.hip -- the pass of a capture stream (stream.hip): tail in segments beside the hot kernel, direct, staged or uploaded.
#include "pass.hpp"

namespace urh {

// Segment boundaries (in chunks) of a streamed pass: S segments on kSegAlign chunks, the last one takes the remainder.
static int segment_bounds(int64_t n_chunks, int wanted, int shape, int last_units, int64_t *bound /*[kMaxSegments + 1]*/) {
    const int64_t blocks = n_chunks / kSegAlign;              // whole alignment units; what is left over belongs to the last segment
    int S = wanted;
    if (S > kMaxSegments) S = kMaxSegments;
    if (S > blocks) S = (int)blocks;
    if (S < 1) S = 1;
    bound[0] = 0;
    if (shape == 1 && S > 2) {
        // halving: 1/2, 1/4, ... of the capture; the last two segments are equal.  The tail of a long first segment runs beside the
        // hot kernel anyway; what is exposed at the end of the capture is the tail of the LAST segment only.
        int64_t left = blocks, at = 0;
        for (int k = 0; k < S - 1; ++k) {
            int64_t take = left / 2;
            const int64_t must_leave = S - 1 - k;             // at least one unit per remaining segment
            if (take < 1) take = 1;
            if (left - take < must_leave) take = left - must_leave;
            at += take; left -= take;
            bound[k + 1] = at * kSegAlign;
        }
    } else if (shape == 2 && S > 1) {
        // S - 1 equal segments and a SHORT last one (last_units alignment units + the remainder): the segments before it run beside the
        // hot kernel; what is exposed behind the hot kernel's end is the last segment's chain of six small kernels, whose length hardly
        // depends on the segment's size (5 - 8 us each) -- so it should be short in the hot kernel's terms too
        int64_t last = last_units < 1 ? 1 : last_units;
        if (last > blocks - (S - 1)) last = blocks - (S - 1);
        const int64_t rest = blocks - last;
        for (int k = 1; k < S; ++k) bound[k] = (rest * k / (S - 1)) * kSegAlign;
    } else {
        for (int k = 1; k < S; ++k) bound[k] = (blocks * k / S) * kSegAlign;
    }
    bound[S] = n_chunks;
    for (int k = 0; k < S; ++k)
        if (bound[k + 1] <= bound[k]) return 0;
    return S;
}

namespace {
struct StreamPass {             // one streamed pass: what its steps (in the order below) hand on to each other
    urhgpu_ctx *ctx; const void *d_iq; int64_t n; const urhgpu_params *p; const urhgpu_outputs *out;
    const void *h_iq;           // upload mode: the capture on the host
    void *host_blob; int64_t cap_host;     // where the tail stores the compact blob (staged: the staging blob in HBM ...
    void *real_host_blob;       // ... and the head still goes here, stored by the pass's last kernel)
    Plan pl; RunArgs a;
    int S; int64_t bound[kMaxSegments + 1]; uint32_t target[kMaxSegments];      // rows segments: chunks [bound[k], bound[k + 1]), their counters' targets
    bool direct, to_stage;
    BitsParams bp; int has_pos; BlobLayout host_layout;
    int slot; uint32_t *progress; SegState *st;
    hipStream_t s; hipEvent_t hot_done;
    ChunkInfo *chunks; uint64_t *slab; void *rs_mem, *scratch; TileTailMem tm; ScanState ss;
    int policy(void *stage_blob);
    int begin();
    int hot();
    int tail(hipEvent_t ev_ready, hipEvent_t ev_rows, int len16);
};
}  // namespace

// Step 1, the policy decision: how many rows segments (S; 0: not a pass for this path -- nothing has been touched), direct, staged.
int StreamPass::policy(void *stage_blob) {
    S = 0;
    int segs = runs_streamable(a) ? segment_bounds(pl.n_chunks, h_iq ? ctx->tune_upload_pieces : ctx->tune_stream_segments, h_iq ? 2 : 0, 1, bound) : 0;
    // DIRECT passes (stream_policy 3, or 4 for the passes that policy 0 would not stream): ONE segment -- the ordinary tail behind the hot
    // kernel (an event, no gate), but rows and packed results are STORED into the pinned host blob by the tail's own kernels: no pack of
    // the whole table at the end, no copy engine, no predicted copy size.
    // Policy 5 (the default): direct when the pass ships no positions (measured, profiles/r04c_ab_direct.txt: 0.294-0.300 ms per
    // pipelined step against 0.306 through pack + copy engine, one capture alone the same as with segments), policy 0 when it does --
    // 5.4 MB of uint32 positions stored over PCIe by a pack kernel take longer than the copy engine needs for the whole blob (0.41 ms).
    // STAGED passes (stream_policy 6; round 6): a direct pass whose "host blob" is a staging blob in HBM (stage_blob, the split layout of
    // compact.hpp: staged_layout); the caller ships it with the copy engine -- the row sections behind ev_rows, i.e. while the bits are
    // still being expanded, the head behind ev_ready.  Why: the row kernel's 1- and 4-byte
    // stores into pinned host memory -- 3.3 MB per GiB as some 10^5 partial-line PCIe writes issued over the 100 us the kernel runs beside
    // the next hot kernel -- cost that hot kernel 10 us per step (profiles/r06b_skips.txt: 0.2855 -> 0.2751 ms without them, the same as
    // without the row kernel altogether); the copy engine's writes do not pass through the shader's memory path.
    int policy = ctx->tune_stream_policy;
    if (policy == 5) policy = (p->write_bit_sample_pos && out->pos && !ctx->tune_stream_pos_direct) ? 0 : (ctx->tune_stream_latency ? 4 : (stage_blob ? 6 : 3));
    if (policy == 6 && !stage_blob) policy = 3;
    direct = to_stage = false;
    if (!h_iq && runs_streamable(a) && host_blob && (policy == 3 || policy == 6)) { direct = true; to_stage = (policy == 6); }
    if (segs < 2 && !direct) return URHGPU_OK;                    // too short to cut, or not the bit-plane kernel's work: the ordinary path
    if (policy == 2 && !h_iq) return URHGPU_OK;
    if ((policy == 0 || policy == 4) && ctx->passes_begun > 0 && !h_iq) {
        // is anything of the pass before still running?  Then this pass's tail will run beside ITS successor's hot kernel as well: one piece
        const hipError_t q = hipEventQuery(ctx->ev_tail[(ctx->flip + 2) % 3]);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            if (policy == 0 || !host_blob) return URHGPU_OK;
            direct = true; to_stage = (stage_blob != nullptr);
        } else if (q != hipSuccess) URH_HIP(q);
    }
    S = segs;
    if (direct) { S = 1; bound[0] = 0; bound[1] = pl.n_chunks; }
    real_host_blob = host_blob;
    if (to_stage) host_blob = stage_blob;
    return URHGPU_OK;
}

// the streams, events and counters of streamed passes: made by the context's first one
static int stream_resources(urhgpu_ctx *ctx) {
    if (ctx->d_seg) return URHGPU_OK;
    URH_HIP(hipMalloc(&ctx->d_seg, 3 * kSegBlockBytes));
    URH_HIP(hipMemset(ctx->d_seg, 0, 3 * kSegBlockBytes));
    URH_HIP(hipDeviceSynchronize());
    URH_HIP(hipStreamCreateWithFlags(&ctx->bits_stream, hipStreamNonBlocking));
    for (int k = 0; k < kMaxSegments; ++k) URH_HIP(hipEventCreateWithFlags(&ctx->ev_piece[k], hipEventDisableTiming));
    for (int k = 0; k < 3; ++k) {
        URH_HIP(hipEventCreateWithFlags(&ctx->ev_hot_done[k], hipEventDisableTiming));
        URH_HIP(hipEventCreateWithFlags(&ctx->ev_bits[k], hipEventDisableTiming));
        for (int j = 0; j < kMaxSegments; ++j) URH_HIP(hipEventCreateWithFlags(&ctx->ev_rows[k][j], hipEventDisableTiming));
    }
    return URHGPU_OK;
}

// Step 2, host / staging layout and scratch: everything that can fail or allocate, BEFORE anything of the pass is queued.
int StreamPass::begin() {
    URH_TRY(stream_resources(ctx));
    // where the rows go on the host: the capacity layout of the compact blob (k_pack_seg) -- checked BEFORE anything of the pass is
    // queued or the arenas rotate (an error return below this point would leave a pass half-begun)
    bp = bits_params(p);
    has_pos = (bp.write_pos && out->pos) ? 1 : 0;
    memset(&host_layout, 0, sizeof(host_layout));
    if (host_blob) {
        const int64_t caps[5] = {out->cap_rows, out->cap_msg, out->cap_bits, out->cap_pos, out->cap_rows};
        host_layout = blob_layout(caps, out->cap_rows, out->cap_bits, out->cap_msg, out->cap_pos, has_pos);
        if (cap_host < host_layout.total) return URHGPU_ERR_CAPACITY;
    }
    URH_TRY(begin_pipelined_pass(ctx));
    slot = ctx->flip;
    progress = (uint32_t *)((char *)ctx->d_seg + (size_t)slot * kSegBlockBytes);
    st = (SegState *)((char *)progress + kMaxSegments * kProgressStride * 4);
    static_assert(kMaxSegments * kProgressStride * 4 + sizeof(SegState) <= kSegBlockBytes && kMaxSegments <= 16, "segment block");
    if (ctx->seg_dirty[slot]) {                                // an earlier pass on this arena died half-way: its counters may not be zero
        URH_HIP(hipDeviceSynchronize());
        URH_HIP(hipMemset(progress, 0, kSegBlockBytes));
        URH_HIP(hipDeviceSynchronize());
        ctx->seg_dirty[slot] = false;
    }
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, out->cap_rows, false, true)));
    ctx->arena.reset();
    ctx->seg_dirty[slot] = true;                               // until the last segment has been queued
    s = ctx->stream;
    URH_TRY(hot_stream_begin(ctx, &s));
    chunks = (ChunkInfo *)ctx->arena.take((size_t)pl.n_chunks * sizeof(ChunkInfo));
    slab = (uint64_t *)ctx->arena.take((size_t)pl.n_chunks * pl.slab_stride * 8);
    rs_mem = ctx->arena.take(resolve_scratch_bytes(pl.n_chunks));
    if (!chunks || !slab || !rs_mem) return URHGPU_ERR_ARG;
    a.chunks = chunks; a.slab = slab;
    // everything that may allocate (and zero) descriptor memory BEFORE anything of the pass is queued
    URH_TRY(tile_tail_mem(ctx, pl.n_chunks, true, &tm));
    const int64_t cap = std::max<int64_t>(out->cap_rows, 1);
    scratch = ctx->arena.take(bits_scratch_bytes(cap));
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(scan_state(ctx, tile_desc_cap(cap, pl.n_chunks), &ss));
    // a segment's counter covers its chunks and the first chunk of the next segment (the resolve kernel's look-ahead), less the first
    // chunk of its own, which the segment before already waited for
    a.progress = progress; a.n_seg = S;
    for (int k = 0; k < S; ++k) {
        const int64_t hi = (k < S - 1) ? bound[k + 1] + 1 : pl.n_chunks, lo = (k == 0) ? 0 : bound[k] + 1;
        a.seg_end[k] = (int32_t)hi;
        target[k] = (uint32_t)(hi - lo);
    }
    return URHGPU_OK;
}

// Step 3, the hot launch: piece by piece behind the capture's upload, or in one
int StreamPass::hot() {
    if (h_iq) {
        // Upload mode (urhgpu_stream_push_upload): the capture arrives from the host in PIECES, and the hot kernel runs piece by piece
        // behind them (RunArgs::launch_lo / launch_hi; a chunk reads the two samples before it: the pieces arrive in order).  Piece k =
        // the chunks of segment k plus the first chunk of segment k + 1 -- the chunk segment k's resolve kernel looks ahead into, so that
        // the segment's tail does not wait for the next piece.  1 GiB over PCIe takes 70 times as long as its hot kernel: what is left
        // behind the last byte's arrival is the last (short) piece's kernel and the last segment's tail.
        // The copies go onto the HOT stream itself: copy 0, kernel 0, copy 1, kernel 1, ...  A stream of their own (copies fully beside
        // the kernels) was measured first and is not robust: HIP maps streams onto a handful of hardware queues, and depending on which
        // streams happened to share one the same pass took 19.4 or 35 ms (tools/upload_probe.py, round 4: the first pipeline of a
        // process was fine, later ones were not).  In one in-order stream a piece's kernel sits between two copies: 283 us of kernels
        // per GiB whatever the number of pieces, plus some 25 us of hand-over per piece -- 1.04 x the bare copy at four pieces.
        // No polling gates here: a gate kernel would spin for the milliseconds a piece takes to arrive; the rows segment of piece k
        // waits for an event behind the piece's hot kernel instead (plain stores in that kernel, no progress counters).
        a.progress = nullptr; a.n_seg = 0;
        const size_t bps = (size_t)dtype_bytes(p->dtype);
        int64_t piece_lo[kMaxSegments], piece_hi[kMaxSegments];
        for (int k = 0; k < S; ++k) {
            piece_lo[k] = k == 0 ? 0 : piece_hi[k - 1];
            piece_hi[k] = (k < S - 1) ? std::min<int64_t>(bound[k + 1] + 1, pl.n_chunks) : pl.n_chunks;
        }
        hipStream_t up = s;
        for (int k = 0; k < S; ++k) {
            {
                const int64_t s0 = piece_lo[k] * pl.chunk_len, s1 = std::min<int64_t>(piece_hi[k] * pl.chunk_len, n);
                URH_HIP(hipMemcpyAsync((char *)const_cast<void *>(d_iq) + (size_t)s0 * bps, (const char *)h_iq + (size_t)s0 * bps, (size_t)(s1 - s0) * bps,
                                       hipMemcpyHostToDevice, up));
            }
            a.launch_lo = piece_lo[k]; a.launch_hi = piece_hi[k];
            const int stl = launch_demod_runs_iq(a, p->dtype, p->mod, out->qad != nullptr, s);
            if (stl != URHGPU_OK) return stl;
            URH_HIP(hipEventRecord(ctx->ev_piece[k], s));
        }
        a.launch_lo = 0; a.launch_hi = 0;
        URH_HIP(hipEventRecord(ctx->ev_hot_done[slot], s));
        hot_done = ctx->ev_hot_done[slot];
        return URHGPU_OK;
    }
    if (direct) { a.progress = nullptr; a.n_seg = 0; }         // (plain stores in the hot kernel, no counters: the tail starts behind its end)
    // the hot kernel's completion: the dispatch's own completion signal where the launcher takes events (an event recorded behind the
    // kernel is one more barrier packet between two hot kernels); nobody waits for it before the last segment has been queued
    return hot_launch(ctx, a, p, true, s, true, ctx->ev_hot_done[slot], nullptr, &hot_done);
}

// Step 4, the tail in segments: rows segments on the tail stream, bits segments on the bits stream behind the rows they expand; neither
// ever waits for the hot kernel as a whole
int StreamPass::tail(hipEvent_t ev_ready, hipEvent_t ev_rows, int len16) {
    const bool event_start = (h_iq != nullptr) || direct;      // the rows segments start behind events, not behind polling gates
    hipStream_t ts = ctx->tail_stream, tb = ctx->bits_stream;
    ResolveArgs r;
    EmitArgs e;
    table_args(ctx, p, pl, n, chunks, slab, rs_mem, out->rows, out->cap_rows, &st->n_acc, &st->rows_at[S - 1], &st->rows_needed, false, &r, &e);
    int8_t *h_state = nullptr; int32_t *h_len = nullptr;
    BitsOut bo{out->bits, out->cap_bits, out->msg_off, out->pauses, out->cap_msg, out->pos, out->cap_pos, out->pos_off, out->counts, out->h_counts};
    if (host_blob) { h_state = (int8_t *)((char *)host_blob + host_layout.off_row_state); h_len = (int32_t *)((char *)host_blob + host_layout.off_row_len); }
    if (to_stage) {
        const StagedLayout SL = staged_layout(out->cap_rows, out->cap_bits, out->cap_msg, out->cap_pos, has_pos);
        h_state = (int8_t *)((char *)host_blob + SL.off_row_state); h_len = (int32_t *)((char *)host_blob + SL.off_row_len);
    }
    // staged passes with 16-bit row lengths: the escape list (count, then pairs) sits in the staging blob's head region, behind the header's place;
    // len16 == 2 (URHGPU_BLOB_ROW16: state and length in one uint16, escapes from 8191 samples on): the list is longer and has a place of
    // its own behind every section of the split layout, in the staging blob while it is built and in the host blob (the caller sized both)
    const bool l16 = to_stage && len16 != 0;
    const bool row16 = l16 && len16 == 2;
    int64_t row16_esc_off = 0;
    if (row16) row16_esc_off = staged_layout(out->cap_rows, out->cap_bits, out->cap_msg, out->cap_pos, has_pos).total;
    int64_t *esc = l16 ? (int64_t *)((char *)host_blob + (row16 ? row16_esc_off : (int64_t)URHGPU_BLOB_HEADER_BYTES)) : nullptr;
    const int64_t esc_cap = row16 ? n / 8191 + 2 : n / 65535 + 2;
    SegPackDst dst{host_blob, cap_host, progress, 0, (direct && ctx->tune_stream_pos_direct) ? 1 : 0, to_stage ? 1 : 0, to_stage ? real_host_blob : nullptr,
                   esc, esc_cap, row16_esc_off};
    // bits segments: the last one is the last rows segment alone (what is exposed behind the hot kernel), the others share the rest
    int Sb = h_iq ? S : 1;       // (an upload: every piece's bits behind its rows -- the pieces are milliseconds apart)
    int bits_end_at[kMaxSegments];                             // bits segment j ends with rows segment bits_end_at[j]
    for (int j = 0; j < Sb - 1; ++j) bits_end_at[j] = (int)((int64_t)(S - 1) * (j + 1) / (Sb - 1)) - 1;
    bits_end_at[Sb - 1] = S - 1;
    int jb = 0;
    int64_t bits_from = 0, scan_b0 = 0;
    // the LAST bits segment goes onto the rows stream, right behind the last rows: no event hop between two
    // streams on the chain that is exposed behind the hot kernel's end; the rows stream then waits for the bits segments before it
    for (int k = 0; k < S; ++k) {
        if (h_iq) URH_HIP(hipStreamWaitEvent(ts, ctx->ev_piece[k], 0));
        else if (direct) URH_HIP(hipStreamWaitEvent(ts, hot_done, 0));
        RowsSegment sg{k, k == S - 1 ? 1 : 0, bound[k], bound[k + 1], SegGate{event_start ? nullptr : progress, k, target[k], k == 0 ? 1 : 0, st, (long long)200000000, 0},
                       h_state, h_len, 1, l16 ? (row16 ? 2 : 1) : 0, esc, esc_cap};
        URH_TRY(launch_rows_segment(r, e, tm, bp, st, sg, ts));
        if (to_stage && ev_rows) URH_HIP(hipEventRecord(ev_rows, ts));      // (one segment: every row section is in the staging blob)
        while (jb < Sb && bits_end_at[jb] < k) ++jb;           // (a bits segment that would end before the first rows segment: none)
        if (jb < Sb && bits_end_at[jb] == k) {
            const bool last = (jb == Sb - 1);
            BitsSegment bs{jb, last ? 1 : 0, bits_from, bound[k + 1], k, st, scan_b0};
            scan_b0 += tile_scan_blocks(bits_from, bound[k + 1], last ? 1 : 0);
            if (last) {
                if (jb > 0) {                                  // behind the bits segments before it (their carries, their packed bytes)
                    URH_HIP(hipEventRecord(ctx->ev_bits[slot], tb));
                    URH_HIP(hipStreamWaitEvent(ts, ctx->ev_bits[slot], 0));
                }
                URH_TRY(launch_bits_segment(tm, bp, bo, scratch, ss, out->rows, out->cap_rows, bs, &dst, ts));
            } else {
                URH_HIP(hipEventRecord(ctx->ev_rows[slot][jb], ts));
                URH_HIP(hipStreamWaitEvent(tb, ctx->ev_rows[slot][jb], 0));
                URH_TRY(launch_bits_segment(tm, bp, bo, scratch, ss, out->rows, out->cap_rows, bs, &dst, tb));
            }
            bits_from = bound[k + 1];
            ++jb;
        }
    }
    URH_HIP(hipGetLastError());
    if (!host_blob) URH_HIP(hipMemsetAsync(progress, 0, kMaxSegments * kProgressStride * 4, ts));       // (nobody else zeroes the counters then)
    ctx->seg_dirty[slot] = false;
    if (ev_ready) URH_HIP(hipEventRecord(ev_ready, ts));         // the host blob is complete
    // the pass is over when the last bits segment has finished (on the rows stream, behind the others) and the hot kernel has retired (its
    // last qad stores): cheap here, the last gate has just seen its last chunk
    URH_HIP(hipStreamWaitEvent(ts, hot_done, 0));
    if (s != ctx->stream && ctx->stream != nullptr) URH_HIP(hipStreamWaitEvent(ctx->stream, hot_done, 0));   // input reuse in stream order
    URH_TRY(end_pipelined_pass(ctx));
    return URHGPU_OK;
}

int iq_to_bits_streamed(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out, void *host_blob,
                        int64_t cap_host, hipEvent_t ev_ready, bool *streamed, const void *h_iq, void *stage_blob, bool *staged, hipEvent_t ev_rows, int len16) {
    *streamed = false;
    if (staged) *staged = false;
    if (!ctx || !p || !out || n <= 0 || !d_iq || !out->rows || !out->counts) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    const bool want_bits = out->bits && out->msg_off && out->pauses && out->pos_off;
    if (!ctx->pipelined || !ctx->tail_stream || n <= 2 || p->mod == URHGPU_MOD_PSK || p->mod == URHGPU_MOD_ASK || !g_tile_tail || !want_bits ||
        (ctx->tune_stream_segments < 2 && !h_iq) || out->cap_rows < 1)
        return URHGPU_OK;
    URH_TRY(check_params(p, true));
    if (((uintptr_t)d_iq & 15) || (out->qad && ((uintptr_t)out->qad & 7))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    StreamPass sp;
    sp.ctx = ctx; sp.d_iq = d_iq; sp.n = n; sp.p = p; sp.out = out; sp.h_iq = h_iq; sp.host_blob = host_blob; sp.cap_host = cap_host;
    sp.pl = make_plan(ctx, n, p->tolerance);
    URH_TRY(hot_run_args(ctx, p, sp.pl, n, 0, true, &sp.a));
    sp.a.in = d_iq; sp.a.qad = out->qad;
    sp.a.lds_pad = ctx->hot_lds_pad;
    if (ctx->wide_int_next) sp.a.wide_int = 1;                // (beside the caller's word: what the stream's probe saw in the captures before)
    URH_TRY(sp.policy(stage_blob));
    if (sp.S == 0) return URHGPU_OK;                          // the ordinary path
    if (sp.to_stage && staged) *staged = true;
    URH_TRY(sp.begin());
    URH_TRY(sp.hot());
    URH_TRY(sp.tail(ev_ready, ev_rows, len16));
    *streamed = true;
    return URHGPU_OK;
}

}  // namespace urh
