// capi_estimators.hip -- estimator and filter passes on device pointers (include/urhgpu.h).
#include "pass.hpp"

using namespace urh;

extern "C" {

// ---- estimator passes (device pointers; see include/urhgpu.h) ---------------------------------------------------
namespace {
__global__ void k_set_i64(int64_t *p, int64_t v) { *p = v; }
}

static int segment_runs_impl(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold,
                             int64_t *d_rows, int64_t cap_rows, int64_t *d_n_rows, float *d_qad_ask) {
    if (!ctx || n < 0 || !d_n_rows || cap_rows < 0) return URHGPU_ERR_ARG;
    if (dtype_bytes(dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    if (n == 0) { URH_HIP(hipMemsetAsync(d_n_rows, 0, 8, ctx->stream)); return URHGPU_OK; }
    if (!d_iq || !d_rows || ((uintptr_t)d_iq & 15)) return URHGPU_ERR_ARG;
    urhgpu_params p;
    memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.mod = URHGPU_MOD_ASK; p.bits_per_symbol = 1; p.center = noise_threshold; p.center_spacing = 0.f;
    p.tolerance = 9;                                   // outlier_tolerance = 10 consecutive samples (auto_interpretation.pyx:72)
    p.samples_per_symbol = 1;
    const Plan pl = make_plan(ctx, n, p.tolerance);
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, cap_rows, false, false)));
    ctx->arena.reset();
    return digitize(ctx, true, d_iq, n, &p, d_qad_ask, d_rows, cap_rows, d_n_rows, ctx->d_counts + 8, ctx->d_counts + 9, pl, 1);
}

int urhgpu_segment_runs_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold,
                            int64_t *d_rows, int64_t cap_rows, int64_t *d_n_rows) {
    return segment_runs_impl(ctx, d_iq, dtype, n, noise_threshold, d_rows, cap_rows, d_n_rows, nullptr);
}

static int message_ranges_impl(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold, int64_t *seg_out, int64_t cap_seg_out,
                               int64_t *n_seg_out, int64_t *merged_out, int64_t cap_merged_out, int64_t *n_merged_out, int *merge_ambiguous,
                               float *d_qad_ask) {
    if (!ctx || n < 0 || !n_seg_out || cap_seg_out < 0 || cap_merged_out < 0 || (cap_seg_out > 0 && !seg_out) || (cap_merged_out > 0 && !merged_out))
        return URHGPU_ERR_ARG;
    if (dtype_bytes(dtype) == 0) return URHGPU_ERR_DTYPE;
    const bool merge = n_merged_out != nullptr;
    *n_seg_out = 0;
    if (merge) *n_merged_out = 0;
    if (merge_ambiguous) *merge_ambiguous = 0;
    if (n == 0 || noise_threshold != noise_threshold) return URHGPU_OK;      // nothing compares greater than NaN: never above the noise
    URH_HIP(hipSetDevice(ctx->device));
    // the state table, the segment table and the message table live in the staging arena for the duration of the call
    const int64_t cap_rows = n / 10 + 2;                   // a state change needs 10 samples in the new state
    const int64_t cap_seg = cap_rows / 2 + 2;
    const size_t need = (size_t)cap_rows * 16 + 2 * (size_t)cap_seg * 16 + seg_scratch_bytes(cap_rows, cap_seg) + seg_ctl_bytes() + 16 * 256;
    URH_TRY(ctx->staging.reserve(need));
    ctx->staging.reset();
    int64_t *d_rows = (int64_t *)ctx->staging.take((size_t)cap_rows * 16);
    // (the control block directly in front of the segment table: the block and the first segments leave in ONE copy)
    const size_t ctl_pad = (seg_ctl_bytes() + 255) & ~size_t(255);
    char *d_ctl_seg = (char *)ctx->staging.take(ctl_pad + (size_t)cap_seg * 16);
    SegCtl *d_ctl = (SegCtl *)d_ctl_seg;
    int64_t *d_seg = d_ctl_seg ? (int64_t *)(d_ctl_seg + ctl_pad) : nullptr;
    int64_t *d_msgs = (int64_t *)ctx->staging.take((size_t)cap_seg * 16);
    void *scratch = ctx->staging.take(seg_scratch_bytes(cap_rows, cap_seg));
    int64_t *d_n_rows = (int64_t *)ctx->staging.take(64);
    if (!d_rows || !d_seg || !d_msgs || !scratch || !d_ctl || !d_n_rows) return URHGPU_ERR_ARG;
    URH_TRY(segment_runs_impl(ctx, d_iq, dtype, n, noise_threshold, d_rows, cap_rows, d_n_rows, d_qad_ask));
    if (d_qad_ask && n <= 2) URH_HIP(hipMemsetAsync(d_qad_ask, 0, (size_t)n * 4, ctx->stream));     // afp_demod of up to two samples: zeros (signal_functions.pyx:335-336)
    URH_TRY(launch_message_ranges(d_rows, d_n_rows, cap_rows, d_iq, dtype, n, noise_threshold, merge ? 1 : 0, d_seg, d_msgs, cap_seg, d_ctl, scratch,
                                  ctx->stream));
    URH_HIP(hipGetLastError());
    // one round trip for the usual case: the control block together with the first segments / merged messages the caller has room for
    // (the counts are not known yet: a prefix of each table is copied speculatively, the rest -- rarely -- afterwards)
    std::vector<char> ctl(seg_ctl_bytes());
    const int64_t spec_seg = std::min<int64_t>(std::min<int64_t>(cap_seg_out, cap_seg), 4096);
    const int64_t spec_mrg = merge ? std::min<int64_t>(std::min<int64_t>(cap_merged_out, cap_seg), 4096) : 0;     // (config 3's capture has 1500 messages: beyond the prefix costs a second round trip)
    std::vector<int64_t> spec_m((size_t)spec_mrg * 2);
    // (through the context's pinned landing zone when it fits: three copies to pageable memory are three synchronous round trips)
    const bool pinned = ctx->h_small && ctl_pad + (size_t)(spec_seg + spec_mrg) * 16 <= kSmallPinned;
    char *l_ctl = pinned ? ctx->h_small : ctl.data();
    int64_t *l_seg = pinned ? (int64_t *)(ctx->h_small + ctl_pad) : seg_out;
    int64_t *l_mrg = pinned ? l_seg + 2 * spec_seg : spec_m.data();
    if (pinned) URH_HIP(hipMemcpyAsync(l_ctl, d_ctl, ctl_pad + (size_t)spec_seg * 16, hipMemcpyDeviceToHost, ctx->stream));
    else {
        URH_HIP(hipMemcpyAsync(l_ctl, d_ctl, ctl.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (spec_seg > 0) URH_HIP(hipMemcpyAsync(l_seg, d_seg, (size_t)spec_seg * 16, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (spec_mrg > 0) URH_HIP(hipMemcpyAsync(l_mrg, d_msgs, (size_t)spec_mrg * 16, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(wait_stream(ctx, ctx->stream));
    if (pinned) {
        memcpy(ctl.data(), l_ctl, ctl.size());
        if (spec_mrg > 0) memcpy(spec_m.data(), l_mrg, (size_t)spec_mrg * 16);
    }
    int64_t n_seg = 0, n_msgs = 0;
    int ambiguous = 0;
    seg_ctl_read(ctl.data(), &n_seg, &n_msgs, &ambiguous);
    if (n_seg > cap_seg) return URHGPU_ERR_CAPACITY;       // cannot happen (a segment needs two state changes)
    *n_seg_out = n_seg;
    const int64_t take = std::min(n_seg, cap_seg_out);
    if (pinned && std::min(take, spec_seg) > 0) memcpy(seg_out, l_seg, (size_t)std::min(take, spec_seg) * 16);
    bool more = false;
    if (take > spec_seg) { URH_HIP(hipMemcpyAsync(seg_out + 2 * spec_seg, d_seg + 2 * spec_seg, (size_t)(take - spec_seg) * 16, hipMemcpyDeviceToHost, ctx->stream)); more = true; }
    if (merge) {
        const bool merged = n_seg > 1;                     // AutoInterpretation.py:108: one segment is returned as it is
        *n_merged_out = merged ? n_msgs : n_seg;
        if (merge_ambiguous) *merge_ambiguous = merged ? ambiguous : 0;
        const int64_t take_m = std::min(*n_merged_out, cap_merged_out);
        if (!merged) {
            // the single segment is the message: it is in seg_out already when the caller has room for a segment, else fetch it
            if (take_m > 0) {
                if (take >= 1) { merged_out[0] = seg_out[0]; merged_out[1] = seg_out[1]; }
                else { URH_HIP(hipMemcpyAsync(merged_out, d_seg, 16, hipMemcpyDeviceToHost, ctx->stream)); more = true; }
            }
        } else {
            const int64_t have = std::min(take_m, spec_mrg);
            if (have > 0) memcpy(merged_out, spec_m.data(), (size_t)have * 16);
            if (take_m > have) { URH_HIP(hipMemcpyAsync(merged_out + 2 * have, d_msgs + 2 * have, (size_t)(take_m - have) * 16, hipMemcpyDeviceToHost, ctx->stream)); more = true; }
        }
    }
    if (more) URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

int urhgpu_message_ranges_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold, int64_t *seg_out, int64_t cap_seg_out,
                              int64_t *n_seg_out, int64_t *merged_out, int64_t cap_merged_out, int64_t *n_merged_out, int *merge_ambiguous) {
    return message_ranges_impl(ctx, d_iq, dtype, n, noise_threshold, seg_out, cap_seg_out, n_seg_out, merged_out, cap_merged_out, n_merged_out,
                               merge_ambiguous, nullptr);
}

int urhgpu_message_ranges_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold, int64_t *seg_out,
                                    int64_t cap_seg_out, int64_t *n_seg_out, int64_t *merged_out, int64_t cap_merged_out, int64_t *n_merged_out,
                                    int *merge_ambiguous, float *d_qad_ask) {
    if (!d_qad_ask || ((uintptr_t)d_qad_ask & 7)) return URHGPU_ERR_ARG;
    if (dtype != URHGPU_DT_F32) return URHGPU_ERR_UNSUPPORTED;
    if (n > 0 && noise_threshold != noise_threshold) return URHGPU_ERR_UNSUPPORTED;     // (no segmentation pass runs for a NaN threshold)
    return message_ranges_impl(ctx, d_iq, dtype, n, noise_threshold, seg_out, cap_seg_out, n_seg_out, merged_out, cap_merged_out, n_merged_out,
                               merge_ambiguous, d_qad_ask);
}

int urhgpu_compact_gt_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float thr, float *d_out, int64_t *d_count) {
    if (!ctx || n < 0 || !d_count || (n > 0 && (!d_x || !d_out))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(compact_scratch_bytes(n) + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(compact_scratch_bytes(n));
    if (!scratch) return URHGPU_ERR_ARG;
    hipLaunchKernelGGL(k_set_i64, dim3(1), dim3(1), 0, ctx->stream, ctx->d_counts + 11, n);
    URH_TRY(launch_compact_gt(d_x, n, ctx->d_counts + 11, thr, d_out, d_count, scratch, ctx->d_tickets, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_edges_le_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float center, int64_t *d_idx, int64_t cap, int64_t *d_count) {
    if (!ctx || n < 0 || cap < 0 || !d_count || (n > 0 && !d_x) || (cap > 0 && !d_idx)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(compact_scratch_bytes(n) + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(compact_scratch_bytes(n));
    if (!scratch) return URHGPU_ERR_ARG;
    hipLaunchKernelGGL(k_set_i64, dim3(1), dim3(1), 0, ctx->stream, ctx->d_counts + 11, n);
    URH_TRY(launch_compact_edges(d_x, n, ctx->d_counts + 11, center, d_idx, cap, d_count, scratch, ctx->d_tickets, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_minmax_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float *d_out2) {
    if (!ctx || n <= 0 || !d_x || !d_out2) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(minmax_scratch_bytes() + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(minmax_scratch_bytes());
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_minmax(d_x, n, d_out2, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_pairwise_sum_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int mode, float mean, float *sum_out) {
    if (!ctx || n < 0 || !sum_out || (n > 0 && !d_x) || (mode != 0 && mode != 1)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    return pairwise_sum_f32(ctx, d_x, n, mode, mean, sum_out);
}

int urhgpu_chunk_power_stats_dev(urhgpu_ctx *ctx, const void *d_src, int dtype, int64_t n_rows, void *d_dst, int64_t n_store, double *sum_out,
                                 double *max_out) {
    if (!ctx || !d_src || n_rows <= 0 || n_rows > (int64_t(1) << 31) || n_store < 0 || n_store > n_rows || !sum_out || !max_out) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    const size_t row = 2 * (size_t)(dtype == URHGPU_DT_F32 ? 4 : (dtype == URHGPU_DT_I16 || dtype == URHGPU_DT_U16) ? 2 : 1);
    if (d_dst == d_src || n_store == 0) d_dst = nullptr;                                   // the chunk already lies where it belongs: statistics only
    if (d_dst && (const char *)d_dst < (const char *)d_src + row * n_rows && (const char *)d_src < (const char *)d_dst + row * n_store) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    if (!ctx->h_chunk) URH_HIP(hipHostMalloc((void **)&ctx->h_chunk, 64));
    const size_t need = chunk_stats_scratch_bytes(dtype, n_rows);
    if (need + 256 > ctx->chunk_work.cap) {
        URH_HIP(hipStreamSynchronize(ctx->stream));
        URH_TRY(ctx->chunk_work.reserve(2 * need + 4096));
    }
    ctx->chunk_work.reset();
    void *scratch = ctx->chunk_work.take(need);
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_chunk_stats(d_src, dtype, n_rows, d_dst, n_store, scratch, ctx->h_chunk, ctx->stream));
    ctx->chunk_launches += 2;
    URH_HIP(hipGetLastError());
    URH_HIP(wait_stream(ctx, ctx->stream));                                // the one synchronisation of a chunk
    if (ctx->h_chunk[2] != 0.0) return URHGPU_ERR_UNSUPPORTED;             // integer total >= 2^53: numpy's float64 sum would round
    *sum_out = ctx->h_chunk[0];
    *max_out = ctx->h_chunk[1];
    return URHGPU_OK;
}

int urhgpu_chunk_stats_launches(urhgpu_ctx *ctx, int64_t *n_launches) {
    if (!ctx || !n_launches) return URHGPU_ERR_ARG;
    *n_launches = (int64_t)ctx->chunk_launches;
    return URHGPU_OK;
}

int urhgpu_histogram_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const double *d_edges, int64_t n_edges, int64_t *d_counts) {
    if (!ctx || n < 0 || n_edges < 2 || n_edges > (1 << 30) || !d_edges || !d_counts || (n > 0 && !d_x)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_hist_edges(d_x, n, d_edges, (int)n_edges, d_counts, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// the FIR's own work area: one per context; a filter on another stream than the last one's waits for that one first
static int fir_work_area(urhgpu_ctx *ctx, size_t bytes, void **work) {
    if (!ctx->ev_fir) URH_HIP(hipEventCreateWithFlags(&ctx->ev_fir, hipEventDisableTiming));
    else if (ctx->fir_stream != ctx->stream || bytes + 1024 > ctx->fir_work.cap) URH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_fir, 0));
    if (bytes + 1024 > ctx->fir_work.cap && ctx->fir_work.cap > 0) URH_HIP(hipEventSynchronize(ctx->ev_fir));      // (growing frees the old area)
    URH_TRY(ctx->fir_work.reserve(bytes + 1024));
    ctx->fir_work.reset();
    *work = ctx->fir_work.take(bytes);
    ctx->fir_stream = ctx->stream;
    return *work ? URHGPU_OK : URHGPU_ERR_ARG;
}

int urhgpu_fir_filter_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const float *d_taps, int64_t m,
                          const float *d_left_halo, float *d_out) {
    if (!ctx || n < 0 || m < 0 || (n > 0 && (!d_x || !d_out)) || (m > 0 && !d_taps)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_taps & 7) || m > (int64_t)1 << 20) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    // The filter's work area (padded taps + the list of tiles handed back: kilobytes) is the context's own, not the rotating arena: on a
    // pipelined context the filter of capture i + 1 then runs BESIDE the tail of pass i instead of behind it (the FIR-halo variant of
    // configs[3] paid filter + hot kernel + tail per step).  The caller's stream is already ordered behind the last pass's HOT kernel
    // (digitize / shard_launch make it wait for that kernel's event), which is what d_out may alias: the capture that kernel read.
    void *work = nullptr;
    URH_TRY(fir_work_area(ctx, fir_work_bytes(n, (int)m), &work));
    URH_TRY(launch_fir((const float2 *)d_x, n, (const float2 *)d_taps, (int)m, (const float2 *)d_left_halo, (float2 *)d_out, ctx->stream, work));
    URH_HIP(hipEventRecord(ctx->ev_fir, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_fir_filter_stats_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const float *d_taps, int64_t m, const float *d_left_halo,
                                float *d_out, int64_t chunk, int64_t n_chunks, double *d_sum, double *d_max) {
    if (!ctx || n <= 0 || m <= 0 || !d_x || !d_out || !d_taps || chunk <= 0 || n_chunks <= 0 || !d_sum || !d_max) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_x & 7) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_taps & 7) || m > (int64_t)1 << 20) return URHGPU_ERR_ARG;
    if (n_chunks * chunk > n || n_chunks > 65535) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    if (chunk < 2048) {          // a tile of outputs would meet more than two chunks: the filter, then the separate statistics pass
        URH_TRY(urhgpu_fir_filter_dev(ctx, d_x, n, d_taps, m, d_left_halo, d_out));
        return urhgpu_magnitude_chunk_stats_dev(ctx, d_out, URHGPU_DT_F32, n, chunk, n_chunks, d_sum, d_max);
    }
    URH_TRY(ctx->arena.reserve(fir_stats_scratch_bytes(n) + fir_work_bytes(n, (int)m) + 2048));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(fir_stats_scratch_bytes(n));
    void *work = ctx->arena.take(fir_work_bytes(n, (int)m));
    if (!scratch || !work) return URHGPU_ERR_ARG;
    URH_TRY(launch_fir((const float2 *)d_x, n, (const float2 *)d_taps, (int)m, (const float2 *)d_left_halo, (float2 *)d_out, ctx->stream, work,
                       chunk, n_chunks, d_sum, d_max, scratch));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_bandpass_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const double *d_taps, int64_t m, int64_t shift,
                        int64_t n_out, const float *d_left, int64_t n_left, const float *d_right, int64_t n_right, void *d_out,
                        int out_c64) {
    if (!ctx || n < 0 || m < 0 || n_out < 0 || n_left < 0 || n_right < 0 || (n > 0 && !d_x) || (m > 0 && !d_taps) ||
        (n_out > 0 && !d_out))
        return URHGPU_ERR_ARG;
    if (((uintptr_t)d_x & 7) || ((uintptr_t)d_taps & 15) || ((uintptr_t)d_out & (out_c64 ? 7 : 15)) || ((uintptr_t)d_left & 7) ||
        ((uintptr_t)d_right & 7) || m > (int64_t)1 << 20 || shift < -((int64_t)1 << 40) || shift > (int64_t)1 << 40)
        return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(bandpass_fft_work_bytes() + 1024));
    ctx->arena.reset();
    void *work = ctx->arena.take(bandpass_fft_work_bytes());
    URH_TRY(launch_bandpass((const float2 *)d_x, n, (const float2 *)d_left, n_left, (const float2 *)d_right, n_right,
                            (const double2 *)d_taps, (int)m, shift, n_out, out_c64 ? nullptr : (double2 *)d_out,
                            out_c64 ? (float2 *)d_out : nullptr, ctx->stream, work));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_magnitude_chunk_stats_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, int64_t chunk, int64_t n_chunks,
                                     double *d_sum, double *d_max) {
    if (!ctx || n < 0 || n_chunks < 0 || (n_chunks > 0 && (!d_iq || !d_sum || !d_max))) return URHGPU_ERR_ARG;
    if (dtype_bytes(dtype) == 0) return URHGPU_ERR_DTYPE;
    if (n_chunks == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(mag_chunk_scratch_bytes(n_chunks) + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(mag_chunk_scratch_bytes(n_chunks));
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_mag_chunk_stats(d_iq, dtype, n, chunk, n_chunks, d_sum, d_max, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// ---- one rank of a sharded capture (shard_estimators.hip) ------------------------------------------------------
int urhgpu_magnitude_chunk_partials_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n_local, int64_t pos_base, int64_t n_total,
                                        int64_t chunk, int64_t n_chunks, double *d_sum, double *d_max) {
    if (!ctx || n_local < 0 || pos_base < 0 || n_total < 0 || pos_base + n_local > n_total || n_chunks < 0 || (n_chunks > 0 && chunk <= 0) ||
        (n_chunks > 0 && (!d_sum || !d_max)) || (n_local > 0 && !d_iq))
        return URHGPU_ERR_ARG;
    if (n_chunks > 0 && n_chunks > n_total / chunk) return URHGPU_ERR_ARG;          // the chunks lie inside the capture
    if (dtype_bytes(dtype) == 0) return URHGPU_ERR_DTYPE;
    if ((uintptr_t)d_iq & (uintptr_t)(dtype_bytes(dtype) - 1)) return URHGPU_ERR_ARG;
    if (n_chunks == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(sp_mag_scratch_bytes(n_chunks) + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(sp_mag_scratch_bytes(n_chunks));
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_mag_chunk_partials(d_iq, dtype, n_local, pos_base, n_total, chunk, n_chunks, d_sum, d_max, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_pairwise_partial_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t m_local, int64_t g_off, int64_t m_total, int mode, float mean,
                                    float *d_out, int64_t cap, int64_t *n_out) {
    if (!ctx || m_local < 0 || g_off < 0 || m_total < 0 || g_off + m_local > m_total || (mode != 0 && mode != 1) || !d_out ||
        ((uintptr_t)d_out & 7) || (m_local > 0 && !d_x) || ((uintptr_t)d_x & 3))
        return URHGPU_ERR_ARG;
    const int64_t words = pairwise_partial_words(m_local, g_off, m_total);
    if (n_out) *n_out = words;
    if (cap < words) return URHGPU_ERR_CAPACITY;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(pairwise_partial_scratch_bytes(m_local) + 1024));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(pairwise_partial_scratch_bytes(m_local));
    if (!scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_pairwise_partial(d_x, m_local, g_off, m_total, mode, mean, d_out, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // extern "C"
