// capi_host.hip -- the host-buffer entry points: stage in, call the device-pointer form, copy the result back.
#include "pass.hpp"

using namespace urh;

extern "C" {

int urhgpu_afp_demod(urhgpu_ctx *ctx, const void *iq, int dtype, int64_t n, float noise_mag, int mod,
                     int mod_order, float costas_loop_bandwidth, float noise_other, float *qad_out) {
    if (!ctx || n < 0 || (n > 0 && (!iq || !qad_out))) return URHGPU_ERR_ARG;
    const int sb = dtype_bytes(dtype);
    if (sb == 0) return URHGPU_ERR_DTYPE;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    urhgpu_params p;
    memset(&p, 0, sizeof(p));
    p.dtype = dtype; p.mod = mod; p.noise_threshold = noise_mag; p.costas_loop_bandwidth = costas_loop_bandwidth;
    p.noise_other = noise_other;
    int bps = 0; while ((1 << (bps + 1)) <= mod_order) ++bps;
    p.bits_per_symbol = bps > 0 ? bps : 1;
    p.samples_per_symbol = 1;
    const size_t in_bytes = (size_t)n * sb, out_bytes = (size_t)n * 4;
    URH_TRY(ctx->staging.reserve(align256(in_bytes) + align256(out_bytes) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, iq, in_bytes, &d_in));
    float *d_out = (float *)ctx->staging.take(out_bytes);
    p.mod_order = mod_order;   // drives the Costas loop order directly (signal_functions.pyx:358)
    URH_TRY(urhgpu_afp_demod_dev(ctx, d_in, n, &p, d_out));
    URH_TRY(fetch_out(ctx, qad_out, d_out, out_bytes));
    return URHGPU_OK;
}

int urhgpu_grab_pulse_lens(urhgpu_ctx *ctx, const float *qad, int64_t n, float center, uint16_t tolerance,
                           int mod, uint32_t samples_per_symbol, uint8_t bits_per_symbol, float center_spacing,
                           float noise_other, int64_t *rows_out, int64_t cap_rows, int64_t *n_rows) {
    if (!ctx || n < 0 || !n_rows || cap_rows < 0) return URHGPU_ERR_ARG;
    *n_rows = 0;
    if (n == 0) return URHGPU_OK;
    if (!qad || (cap_rows > 0 && !rows_out)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    urhgpu_params p;
    memset(&p, 0, sizeof(p));
    p.dtype = URHGPU_DT_F32; p.mod = mod; p.bits_per_symbol = bits_per_symbol; p.center = center;
    p.center_spacing = center_spacing; p.tolerance = tolerance; p.samples_per_symbol = samples_per_symbol;
    p.noise_other = noise_other;
    if (bits_per_symbol < 1 || bits_per_symbol > 7) return URHGPU_ERR_UNSUPPORTED;
    // worst case one row per (tolerance+1) samples; stage at that size on the device, copy what fits
    const int64_t dev_cap = n / ((int64_t)tolerance + 1) + 2;
    URH_TRY(ctx->staging.reserve(align256((size_t)n * 4) + align256((size_t)dev_cap * 16) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, qad, (size_t)n * 4, &d_in));
    int64_t *d_rows = (int64_t *)ctx->staging.take((size_t)dev_cap * 16);
    int64_t *d_n = ctx->d_counts + 10;
    URH_TRY(urhgpu_grab_pulse_lens_dev(ctx, (const float *)d_in, n, &p, d_rows, dev_cap, d_n));
    URH_TRY(fetch_out(ctx, ctx->h_counts, d_n, 8));
    const int64_t rows = ctx->h_counts[0];
    *n_rows = rows;
    if (rows > cap_rows) return URHGPU_ERR_CAPACITY;
    if (rows > 0) {
        URH_TRY(fetch_out(ctx, rows_out, d_rows, (size_t)rows * 16));
    }
    return URHGPU_OK;
}

int urhgpu_ppseq_to_bits(urhgpu_ctx *ctx, const int64_t *rows, int64_t n_rows, int64_t samples_per_symbol,
                         int bits_per_symbol, int write_pos, int64_t pause_threshold,
                         uint8_t *bits, int64_t cap_bits, int64_t *msg_off, int64_t *pauses, int64_t cap_msg,
                         int64_t *pos, int64_t cap_pos, int64_t *pos_off, int64_t *counts) {
    if (!ctx || n_rows < 0 || !counts || !msg_off || !pos_off || samples_per_symbol < 1 || bits_per_symbol < 1)
        return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    urhgpu_params p;
    memset(&p, 0, sizeof(p));
    p.samples_per_symbol = (uint32_t)samples_per_symbol; p.bits_per_symbol = bits_per_symbol;
    p.pause_threshold = pause_threshold; p.write_bit_sample_pos = write_pos;
    const int64_t cb = std::max<int64_t>(cap_bits, 1), cm = std::max<int64_t>(cap_msg, 1), cp = std::max<int64_t>(cap_pos, 1);
    const size_t need = align256((size_t)std::max<int64_t>(n_rows, 1) * 16) + align256((size_t)cb) + 3 * align256((size_t)(cm + 1) * 8) +
                        align256((size_t)cp * 8) + 4096;
    URH_TRY(ctx->staging.reserve(need));
    ctx->staging.reset();
    void *d_rows = nullptr;
    URH_TRY(stage_in(ctx, rows, (size_t)n_rows * 16, &d_rows));
    urhgpu_outputs o;
    memset(&o, 0, sizeof(o));
    o.bits = (uint8_t *)ctx->staging.take((size_t)cb); o.cap_bits = cap_bits;
    o.msg_off = (int64_t *)ctx->staging.take((size_t)(cm + 1) * 8);
    o.pauses = (int64_t *)ctx->staging.take((size_t)(cm + 1) * 8); o.cap_msg = cap_msg;
    o.pos_off = (int64_t *)ctx->staging.take((size_t)(cm + 1) * 8);
    o.pos = (int64_t *)ctx->staging.take((size_t)cp * 8); o.cap_pos = cap_pos;
    o.counts = ctx->d_counts;
    int64_t *d_n = ctx->d_counts + 10;
    ctx->h_counts[8] = n_rows;
    URH_HIP(hipMemcpyAsync(d_n, ctx->h_counts + 8, 8, hipMemcpyHostToDevice, ctx->stream));
    URH_TRY(urhgpu_ppseq_to_bits_dev(ctx, (const int64_t *)d_rows, d_n, n_rows, &p, &o));
    URH_TRY(fetch_out(ctx, ctx->h_counts, ctx->d_counts, 4 * 8));
    const int64_t n_msg = ctx->h_counts[1], n_bits = ctx->h_counts[2], n_pos = ctx->h_counts[3];
    counts[0] = n_msg; counts[1] = n_bits; counts[2] = n_pos;
    if (n_msg > cap_msg || n_bits > cap_bits || (write_pos && n_pos > cap_pos)) return URHGPU_ERR_CAPACITY;
    if (n_bits) URH_HIP(hipMemcpyAsync(bits, o.bits, (size_t)n_bits, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipMemcpyAsync(msg_off, o.msg_off, (size_t)(n_msg + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipMemcpyAsync(pos_off, o.pos_off, (size_t)(n_msg + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (n_msg) URH_HIP(hipMemcpyAsync(pauses, o.pauses, (size_t)n_msg * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (write_pos && n_pos) URH_HIP(hipMemcpyAsync(pos, o.pos, (size_t)n_pos * 8, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    return URHGPU_OK;
}

int urhgpu_fir_filter(urhgpu_ctx *ctx, const float *x, int64_t n, const float *taps, int64_t m, float *out) {
    if (!ctx || n < 0 || m < 0 || (n > 0 && (!x || !out)) || (m > 0 && !taps)) return URHGPU_ERR_ARG;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(ctx->staging.reserve(2 * align256((size_t)n * 8) + align256((size_t)std::max<int64_t>(m, 1) * 8) + 1024));
    ctx->staging.reset();
    void *d_x = nullptr, *d_t = nullptr;
    URH_TRY(stage_in(ctx, x, (size_t)n * 8, &d_x));
    URH_TRY(stage_in(ctx, taps, (size_t)m * 8, &d_t));
    float *d_out = (float *)ctx->staging.take((size_t)n * 8);
    if (!d_out) return URHGPU_ERR_ARG;
    URH_TRY(urhgpu_fir_filter_dev(ctx, (const float *)d_x, n, (const float *)d_t, m, nullptr, d_out));
    URH_TRY(fetch_out(ctx, out, d_out, (size_t)n * 8));
    return URHGPU_OK;
}

int urhgpu_bandpass(urhgpu_ctx *ctx, const float *x, int64_t n, const double *taps, int64_t m, int64_t shift, int64_t n_out,
                    double *out) {
    if (!ctx || n < 0 || m < 0 || n_out < 0 || (n > 0 && !x) || (m > 0 && !taps) || (n_out > 0 && !out)) return URHGPU_ERR_ARG;
    if (n_out == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(ctx->staging.reserve(align256((size_t)std::max<int64_t>(n, 1) * 8) + align256((size_t)std::max<int64_t>(m, 1) * 16) +
                                 align256((size_t)n_out * 16) + 1024));
    ctx->staging.reset();
    void *d_x = nullptr, *d_t = nullptr;
    URH_TRY(stage_in(ctx, x, (size_t)n * 8, &d_x));
    URH_TRY(stage_in(ctx, taps, (size_t)m * 16, &d_t));
    double *d_out = (double *)ctx->staging.take((size_t)n_out * 16);
    if (!d_out) return URHGPU_ERR_ARG;
    URH_TRY(urhgpu_bandpass_dev(ctx, (const float *)d_x, n, (const double *)d_t, m, shift, n_out, nullptr, 0, nullptr, 0, d_out, 0));
    URH_TRY(fetch_out(ctx, out, d_out, (size_t)n_out * 16));
    return URHGPU_OK;
}

int urhgpu_iir_filter(urhgpu_ctx *ctx, const double *a, int64_t na, const double *b, int64_t nb, const float *x, int64_t n,
                      float *out) {
    if (!ctx || n < 0 || na < 0 || nb < 0 || (n > 0 && (!x || !out)) || (na > 0 && !a) || (nb > 0 && !b)) return URHGPU_ERR_ARG;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(ctx->staging.reserve(2 * align256((size_t)n * 8) + align256((size_t)(na + 1) * 8) + align256((size_t)(nb + 1) * 8) + 1024));
    ctx->staging.reset();
    void *d_x = nullptr, *d_a = nullptr, *d_b = nullptr;
    URH_TRY(stage_in(ctx, x, (size_t)n * 8, &d_x));
    URH_TRY(stage_in(ctx, a, (size_t)na * 8, &d_a));
    URH_TRY(stage_in(ctx, b, (size_t)nb * 8, &d_b));
    float *d_out = (float *)ctx->staging.take((size_t)n * 8);
    if (!d_out) return URHGPU_ERR_ARG;
    URH_TRY(launch_iir((const double *)d_a, na, (const double *)d_b, nb, (const float2 *)d_x, n, (float2 *)d_out, ctx->stream));
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, out, d_out, (size_t)n * 8));
    return URHGPU_OK;
}

int urhgpu_get_magnitudes(urhgpu_ctx *ctx, const void *iq, int dtype, int64_t n, double *out) {
    if (!ctx || n < 0 || (n > 0 && (!iq || !out))) return URHGPU_ERR_ARG;
    const int sb = dtype_bytes(dtype);
    if (sb == 0) return URHGPU_ERR_DTYPE;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(ctx->staging.reserve(align256((size_t)n * sb) + align256((size_t)n * 8) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, iq, (size_t)n * sb, &d_in));
    double *d_out = (double *)ctx->staging.take((size_t)n * 8);
    if (!d_out) return URHGPU_ERR_ARG;
    URH_TRY(launch_magnitudes(d_in, dtype, n, d_out, ctx->stream));
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, out, d_out, (size_t)n * 8));
    return URHGPU_OK;
}

// ---- host-array forms of the reference's util / auto_interpretation functions on the path (urh_amd/util.py, auto_interpretation.py) ----
int urhgpu_minmax(urhgpu_ctx *ctx, const void *arr, int dtype, int64_t n, void *out2) {
    if (!ctx || n < 0 || !out2 || (n > 0 && !arr)) return URHGPU_ERR_ARG;
    const int vb = value_bytes(dtype);
    if (vb == 0) return URHGPU_ERR_DTYPE;
    if (n == 0) { memset(out2, 0, 2 * (size_t)vb); return URHGPU_OK; }              // util.pyx:22-23: (0, 0)
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->staging.reserve(align256((size_t)n * vb) + align256(minmax_scratch_bytes()) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, arr, (size_t)n * vb, &d_in));
    void *scratch = ctx->staging.take(minmax_scratch_bytes());
    void *d_out = ctx->staging.take(64);
    if (!scratch || !d_out) return URHGPU_ERR_ARG;
    URH_TRY(launch_minmax_any(d_in, dtype, n, d_out, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, out2, d_out, 2 * (size_t)vb));
    return URHGPU_OK;
}

int urhgpu_segment_messages(urhgpu_ctx *ctx, const void *magnitudes, int is_f64, int64_t n, float noise_threshold, int64_t *seg_out,
                            int64_t cap_seg, int64_t *n_seg) {
    if (!ctx || n < 0 || !n_seg || cap_seg < 0 || (n > 0 && !magnitudes) || (cap_seg > 0 && !seg_out)) return URHGPU_ERR_ARG;
    *n_seg = 0;
    if (n == 0 || noise_threshold != noise_threshold) return URHGPU_OK;           // nothing compares greater than NaN
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    const size_t eb = is_f64 ? 8 : 4;
    const int64_t cap_rows = n / 10 + 2, cap = cap_rows / 2 + 2;
    // magnitudes and flags live in the aux arena (urhgpu_segment_runs' digitize uses the main one), tables in the staging arena
    URH_TRY(ctx->aux.reserve(align256((size_t)n * eb) + align256((size_t)n * 4) + 1024));
    ctx->aux.reset();
    void *d_mag = ctx->aux.take((size_t)n * eb);
    float *d_flags = (float *)ctx->aux.take((size_t)n * 4);
    URH_TRY(ctx->staging.reserve((size_t)cap_rows * 16 + 2 * (size_t)cap * 16 + seg_scratch_bytes(cap_rows, cap) + seg_ctl_bytes() + 16 * 256));
    ctx->staging.reset();
    int64_t *d_rows = (int64_t *)ctx->staging.take((size_t)cap_rows * 16);
    int64_t *d_seg = (int64_t *)ctx->staging.take((size_t)cap * 16);
    int64_t *d_msgs = (int64_t *)ctx->staging.take((size_t)cap * 16);
    void *scratch = ctx->staging.take(seg_scratch_bytes(cap_rows, cap));
    SegCtl *d_ctl = (SegCtl *)ctx->staging.take(seg_ctl_bytes());
    int64_t *d_n_rows = (int64_t *)ctx->staging.take(64);
    if (!d_mag || !d_flags || !d_rows || !d_seg || !d_msgs || !scratch || !d_ctl || !d_n_rows) return URHGPU_ERR_ARG;
    URH_HIP(hipMemcpyAsync(d_mag, magnitudes, (size_t)n * eb, hipMemcpyHostToDevice, ctx->stream));
    URH_TRY(launch_above_flags(d_mag, is_f64, n, noise_threshold, d_flags, ctx->stream));
    urhgpu_params p;
    memset(&p, 0, sizeof(p));
    p.dtype = URHGPU_DT_F32; p.mod = URHGPU_MOD_ASK; p.bits_per_symbol = 1; p.center = 0.5f; p.center_spacing = 0.f;
    p.tolerance = 9;                                   // outlier_tolerance = 10 consecutive samples (auto_interpretation.pyx:72)
    p.samples_per_symbol = 1;
    const Plan pl = make_plan(ctx, n, p.tolerance);
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, cap_rows, false, false)));
    ctx->arena.reset();
    URH_TRY(digitize(ctx, false, d_flags, n, &p, nullptr, d_rows, cap_rows, d_n_rows, ctx->d_counts + 8, ctx->d_counts + 9, pl, 1));
    URH_TRY(launch_message_ranges(d_rows, d_n_rows, cap_rows, d_flags, kDtAboveFlags, n, 0.5f, 0, d_seg, d_msgs, cap, d_ctl, scratch, ctx->stream));
    URH_HIP(hipGetLastError());
    std::vector<char> ctl(seg_ctl_bytes());
    URH_TRY(fetch_out(ctx, ctl.data(), d_ctl, ctl.size()));
    int64_t ns = 0, nm = 0;
    int amb = 0;
    seg_ctl_read(ctl.data(), &ns, &nm, &amb);
    *n_seg = ns;
    if (ns > cap_seg) return URHGPU_ERR_CAPACITY;
    if (ns > 0) {
        URH_TRY(fetch_out(ctx, seg_out, d_seg, (size_t)ns * 16));
    }
    return URHGPU_OK;
}

int urhgpu_get_plateau_lengths(urhgpu_ctx *ctx, const float *rect_data, int64_t n, float center, int percentage, uint64_t *out, int64_t cap,
                               int64_t *n_out) {
    if (!ctx || n < 0 || !n_out || cap < 0 || percentage < 0 || (n > 0 && !rect_data) || (cap > 0 && !out)) return URHGPU_ERR_ARG;
    *n_out = 0;
    if (n == 0) return URHGPU_OK;                              // auto_interpretation.pyx:180-181
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->aux.reserve(align256((size_t)n * 4) + 1024));
    ctx->aux.reset();
    float *d_x = (float *)ctx->aux.take((size_t)n * 4);
    if (!d_x) return URHGPU_ERR_ARG;
    URH_HIP(hipMemcpyAsync(d_x, rect_data, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int64_t range[2] = {0, n};
    const double c = (double)center;
    int64_t off[2] = {0, 0};
    // boundaries are searched in the first percentage % + a window that doubles until it holds one beyond the mark (or the signal ends)
    for (int64_t extra = int64_t(1) << 16;; extra *= 2) {
        const int st = urhgpu_msg_plateaus(ctx, d_x, n, range, &c, 1, percentage, extra, off, out, cap);
        if (st == URHGPU_ERR_CAPACITY) { *n_out = off[1]; return st; }
        URH_TRY(st);
        if (off[1] >= 0) break;
        if (extra >= n) { off[1] = -off[1] - 1; break; }
    }
    *n_out = off[1];
    return URHGPU_OK;
}

int urhgpu_median_filter(urhgpu_ctx *ctx, const double *data, int64_t n, unsigned int k, float *out) {
    if (!ctx || n < 0 || (n > 0 && (!data || !out))) return URHGPU_ERR_ARG;
    if (k < 1 || k > 64) return URHGPU_ERR_UNSUPPORTED;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->staging.reserve(align256((size_t)n * 8) + align256((size_t)n * 4) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, data, (size_t)n * 8, &d_in));
    float *d_out = (float *)ctx->staging.take((size_t)n * 4);
    if (!d_out) return URHGPU_ERR_ARG;
    URH_TRY(launch_median_filter((const double *)d_in, n, (int)k, d_out, ctx->stream));
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, out, d_out, (size_t)n * 4));
    return URHGPU_OK;
}

int urhgpu_dc_correct(urhgpu_ctx *ctx, const void *h_in, int64_t n, int dtype, void *h_out, void *h_mean) {
    if (!ctx || n < 0 || (n > 0 && (!h_in || !h_out))) return URHGPU_ERR_ARG;
    const int sb = dtype_bytes(dtype);
    if (sb == 0) return URHGPU_ERR_DTYPE;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * sb, mean_bytes = dtype == URHGPU_DT_F32 ? 8 : 16;
    URH_TRY(ctx->staging.reserve(2 * align256(bytes) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, h_in, bytes, &d_in));
    void *d_out = ctx->staging.take(bytes), *d_mean = ctx->staging.take(16);
    if (!d_out || !d_mean) return URHGPU_ERR_ARG;
    URH_TRY(urhgpu_dc_correct_dev(ctx, d_in, n, dtype, d_out, d_mean));
    if (h_mean) URH_HIP(hipMemcpyAsync(h_mean, d_mean, mean_bytes, hipMemcpyDeviceToHost, ctx->stream));
    URH_TRY(fetch_out(ctx, h_out, d_out, bytes));
    return URHGPU_OK;
}

}  // extern "C"
