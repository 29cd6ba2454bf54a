// capi_misc.hip -- modulation, spectrogram, conversions, FFT peak, plot paths, .sub run lengths (include/urhgpu.h).
#include "pass.hpp"

using namespace urh;

extern "C" {

// mod: URHGPU_MOD_ASK / _FSK / _PSK / _OQPSK, or urh::kModGfsk with the Gaussian taps (and optionally the caller's filtered
// frequencies, one float per data sample of every message, back to back)
static int modulate_common(urhgpu_ctx *ctx, const uint8_t *bits, const int64_t *bit_off, const uint32_t *pause, const uint32_t *start,
                           int n_msgs, uint32_t samples_per_symbol, int mod, const float *parameters, int bits_per_symbol,
                           float carrier_amplitude, float carrier_frequency, float carrier_phase, float sample_rate, int dtype,
                           const float *gauss_fir, int n_taps, const float *frequencies,
                           void *d_out, int64_t cap_samples, int64_t *total_samples) {
    const bool gfsk = (mod == urh::kModGfsk);
    if (gfsk && (!gauss_fir || n_taps < 1)) return URHGPU_ERR_ARG;
    if (!ctx || n_msgs < 0 || !total_samples || (n_msgs > 0 && (!bit_off || !pause || !start || !parameters))) return URHGPU_ERR_ARG;
    const bool oqpsk = (mod == URHGPU_MOD_OQPSK);
    if (mod != URHGPU_MOD_ASK && mod != URHGPU_MOD_FSK && mod != URHGPU_MOD_PSK && !oqpsk && !gfsk) return URHGPU_ERR_UNSUPPORTED;
    if (oqpsk && bits_per_symbol != 2) return URHGPU_ERR_ARG;                    // assert bits_per_symbol == 2 (:120)
    if (dtype != URHGPU_DT_F32 && dtype != URHGPU_DT_I8 && dtype != URHGPU_DT_I16) return URHGPU_ERR_DTYPE;
    if (bits_per_symbol < 1 || bits_per_symbol > 16 || samples_per_symbol == 0 || n_msgs > 65535) return URHGPU_ERR_UNSUPPORTED;
    std::vector<ModMsg> msgs((size_t)n_msgs);
    int64_t total = 0, total_sym = 0, max_samples = 0;
    for (int m = 0; m < n_msgs; ++m) {
        const int64_t nb = bit_off[m + 1] - bit_off[m];
        if (nb < 0) return URHGPU_ERR_ARG;
        // GFSK re-derives bits_per_symbol as len(bits) // num_symbols (:201): no whole symbol -> ZeroDivisionError there;
        // a message shorter than bits_per_symbol symbols can derive a larger value: not supported
        if (gfsk && nb > 0 && (nb / bits_per_symbol == 0 || nb / (nb / bits_per_symbol) != bits_per_symbol))
            return nb / bits_per_symbol == 0 ? URHGPU_ERR_ARG : URHGPU_ERR_UNSUPPORTED;
        ModMsg &g = msgs[(size_t)m];
        g.bit_off = bit_off[m]; g.n_sym = nb / bits_per_symbol; g.sym_off = total_sym; g.out_off = total;
        g.pause = pause[m]; g.start = start[m];
        const int64_t ns = g.n_sym * (int64_t)samples_per_symbol + pause[m];
        total += ns; total_sym += g.n_sym;
        max_samples = std::max(max_samples, ns);
    }
    *total_samples = total;
    if (total > cap_samples) return URHGPU_ERR_CAPACITY;
    if (total == 0) return URHGPU_OK;
    if (!d_out || !bits) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    const int64_t n_bits = bit_off[n_msgs];
    const size_t n_par = (size_t)1 << bits_per_symbol;
    URH_TRY(ctx->staging.reserve(align256((size_t)std::max<int64_t>(n_bits, 1)) + align256(msgs.size() * sizeof(ModMsg)) +
                                 align256(n_par * 4) + align256((size_t)std::max<int64_t>(total_sym, 1) * 4) + 2048 +
                                 (gfsk ? align256((size_t)n_taps * 4) + 2 * align256((size_t)std::max<int64_t>(total_sym, 1) * samples_per_symbol * 4) : 0)));
    ctx->staging.reset();
    void *d_bits = nullptr, *d_msgs = nullptr, *d_par = nullptr;
    std::vector<uint8_t> oq;
    if (oqpsk) {
        // get_oqpsk_bits (:179-194) per message: even bits stay, odd bits are delayed by one symbol; of the num_bits + 2
        // bits it returns the symbol loop reads the first 2 * n_sym (total_symbols is taken from the original length)
        oq.assign((size_t)n_bits, 0);
        for (int m = 0; m < n_msgs; ++m) {
            const uint8_t *b = bits + bit_off[m];
            uint8_t *r = oq.data() + bit_off[m];
            const int64_t nb = bit_off[m + 1] - bit_off[m];
            if (nb == 0) continue;
            r[0] = b[0];
            for (int64_t i = 2; i < nb - 2; i += 2) { r[i] = b[i]; r[i + 1] = b[i - 1]; }
        }
        bits = oq.data();
    }
    URH_TRY(stage_in(ctx, bits, (size_t)n_bits, &d_bits));
    URH_TRY(stage_in(ctx, msgs.data(), msgs.size() * sizeof(ModMsg), &d_msgs));
    URH_TRY(stage_in(ctx, parameters, n_par * 4, &d_par));
    float *d_phase = (float *)ctx->staging.take((size_t)std::max<int64_t>(total_sym, 1) * 4);
    if (!d_phase) return URHGPU_ERR_ARG;
    ModArgs a;
    a.bits = (const uint8_t *)d_bits; a.msgs = (const ModMsg *)d_msgs; a.params = (const float *)d_par; a.phase = d_phase;
    a.out = d_out; a.n_msgs = n_msgs; a.mod = oqpsk ? URHGPU_MOD_PSK : mod; a.oqpsk = oqpsk ? 1 : 0; a.dtype = dtype; a.bps = bits_per_symbol; a.sps = samples_per_symbol;
    a.carrier_amplitude = carrier_amplitude; a.carrier_frequency = carrier_frequency; a.carrier_phase = carrier_phase;
    a.sample_rate = sample_rate;
    a.taps = nullptr; a.n_taps = 0; a.freq_given = 0; a.gf_freq = a.gf_phase = nullptr;
    if (gfsk) {
        const size_t n_data = (size_t)total_sym * samples_per_symbol;
        void *d_taps = nullptr;
        URH_TRY(stage_in(ctx, gauss_fir, (size_t)n_taps * 4, &d_taps));
        a.taps = (const float *)d_taps; a.n_taps = n_taps;
        if (frequencies && n_data) {
            void *d_f = nullptr;
            URH_TRY(stage_in(ctx, frequencies, n_data * 4, &d_f));
            a.gf_freq = (float *)d_f; a.freq_given = 1;
        } else {
            a.gf_freq = (float *)ctx->staging.take(std::max<size_t>(n_data, 1) * 4);
        }
        a.gf_phase = (float *)ctx->staging.take(std::max<size_t>(n_data, 1) * 4);
        if (!a.gf_freq || !a.gf_phase) return URHGPU_ERR_ARG;
    }
    URH_TRY(launch_modulate(a, max_samples, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_modulate_dev(urhgpu_ctx *ctx, const uint8_t *bits, const int64_t *bit_off, const uint32_t *pause, const uint32_t *start,
                        int n_msgs, uint32_t samples_per_symbol, int mod, const float *parameters, int bits_per_symbol,
                        float carrier_amplitude, float carrier_frequency, float carrier_phase, float sample_rate, int dtype,
                        void *d_out, int64_t cap_samples, int64_t *total_samples) {
    if (mod == urh::kModGfsk) return URHGPU_ERR_UNSUPPORTED;
    return modulate_common(ctx, bits, bit_off, pause, start, n_msgs, samples_per_symbol, mod, parameters, bits_per_symbol, carrier_amplitude,
                           carrier_frequency, carrier_phase, sample_rate, dtype, nullptr, 0, nullptr, d_out, cap_samples, total_samples);
}

int urhgpu_modulate_gfsk_dev(urhgpu_ctx *ctx, const uint8_t *bits, const int64_t *bit_off, const uint32_t *pause, const uint32_t *start,
                             int n_msgs, uint32_t samples_per_symbol, const float *parameters, int bits_per_symbol,
                             float carrier_amplitude, float carrier_phase, float sample_rate, int dtype, const float *gauss_fir,
                             int n_taps, const float *frequencies, void *d_out, int64_t cap_samples, int64_t *total_samples) {
    return modulate_common(ctx, bits, bit_off, pause, start, n_msgs, samples_per_symbol, urh::kModGfsk, parameters, bits_per_symbol,
                           carrier_amplitude, 0.0f, carrier_phase, sample_rate, dtype, gauss_fir, n_taps, frequencies, d_out, cap_samples,
                           total_samples);
}

static int modulate_one(urhgpu_ctx *ctx, const uint8_t *bits, int64_t num_bits, uint32_t samples_per_symbol, int mod,
                        const float *parameters, int bits_per_symbol, float carrier_amplitude, float carrier_frequency,
                        float carrier_phase, float sample_rate, uint32_t pause, uint32_t start, int dtype, const float *gauss_fir,
                        int n_taps, const float *frequencies, void *out) {
    if (!ctx || num_bits < 0 || bits_per_symbol < 1) return URHGPU_ERR_ARG;
    if (dtype != URHGPU_DT_F32 && dtype != URHGPU_DT_I8 && dtype != URHGPU_DT_I16) return URHGPU_ERR_DTYPE;
    const int64_t total = (num_bits / bits_per_symbol) * (int64_t)samples_per_symbol + pause;
    if (total == 0) return URHGPU_OK;
    if (!out) return URHGPU_ERR_ARG;
    const size_t bytes = (size_t)total * 2 * (dtype == URHGPU_DT_F32 ? 4 : (dtype == URHGPU_DT_I8 ? 1 : 2));
    if (num_bits == 0) { memset(out, 0, bytes); return URHGPU_OK; }             // np.zeros, :104-106
    URH_HIP(hipSetDevice(ctx->device));
    void *d_out = nullptr;                                 // not from the staging arena: urhgpu_modulate_dev resets it
    URH_HIP(hipMalloc(&d_out, bytes));
    const int64_t off[2] = {0, num_bits};
    int64_t got = 0;
    int st = modulate_common(ctx, bits, off, &pause, &start, 1, samples_per_symbol, mod, parameters, bits_per_symbol,
                             carrier_amplitude, carrier_frequency, carrier_phase, sample_rate, dtype, gauss_fir, n_taps, frequencies,
                             d_out, total, &got);
    if (st == URHGPU_OK) {
        hipError_t e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) st = urh::hip_fail(e, "modulate D2H", __FILE__, __LINE__);
    }
    (void)hipFree(d_out);
    return st;
}

int urhgpu_modulate(urhgpu_ctx *ctx, const uint8_t *bits, int64_t num_bits, uint32_t samples_per_symbol, int mod,
                    const float *parameters, int bits_per_symbol, float carrier_amplitude, float carrier_frequency,
                    float carrier_phase, float sample_rate, uint32_t pause, uint32_t start, int dtype, void *out) {
    if (mod == urh::kModGfsk) return URHGPU_ERR_UNSUPPORTED;
    return modulate_one(ctx, bits, num_bits, samples_per_symbol, mod, parameters, bits_per_symbol, carrier_amplitude, carrier_frequency,
                        carrier_phase, sample_rate, pause, start, dtype, nullptr, 0, nullptr, out);
}

int urhgpu_modulate_gfsk(urhgpu_ctx *ctx, const uint8_t *bits, int64_t num_bits, uint32_t samples_per_symbol, const float *parameters,
                         int bits_per_symbol, float carrier_amplitude, float carrier_phase, float sample_rate, uint32_t pause,
                         uint32_t start, int dtype, const float *gauss_fir, int n_taps, const float *frequencies, void *out) {
    return modulate_one(ctx, bits, num_bits, samples_per_symbol, urh::kModGfsk, parameters, bits_per_symbol, carrier_amplitude, 0.0f,
                        carrier_phase, sample_rate, pause, start, dtype, gauss_fir, n_taps, frequencies, out);
}

int urhgpu_spectrogram_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int window_size, int64_t hop, int64_t frames,
                           const double *d_window, const double *d_twiddles, double *d_stft, float *d_db) {
    if (!ctx || !d_x || n < 0 || !d_window || !d_twiddles || ((d_stft != nullptr) == (d_db != nullptr))) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_x & 7) || ((uintptr_t)d_twiddles & 15) || ((uintptr_t)d_stft & 15)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_stft((const float2 *)d_x, n, window_size, hop, frames, d_window, (const double2 *)d_twiddles, (double2 *)d_stft, d_db,
                        ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_bgra_lookup_dev(urhgpu_ctx *ctx, const float *d_db, int64_t frames, int window_size, const uint32_t *d_colormap,
                           int n_colors, float data_min, float data_max, uint32_t *d_image) {
    if (!ctx || !d_db || !d_colormap || !d_image || frames < 0 || window_size < 1) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_bgra_lookup(d_db, frames, window_size, d_colormap, n_colors, data_min, data_max, d_image, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// convert_to (scaling) and astype (plain casts) differ in their kernel only
static int convert_with(decltype(&launch_convert) launch, urhgpu_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, int64_t n) {
    if (!ctx || n < 0 || (n > 0 && (!d_src || !d_dst))) return URHGPU_ERR_ARG;
    if (src_dtype == dst_dtype) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch(d_src, src_dtype, d_dst, dst_dtype, n, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}
int urhgpu_convert_dev(urhgpu_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, int64_t n) {
    return convert_with(launch_convert, ctx, d_src, src_dtype, d_dst, dst_dtype, n);
}
int urhgpu_astype_dev(urhgpu_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, int64_t n) {
    return convert_with(launch_astype, ctx, d_src, src_dtype, d_dst, dst_dtype, n);
}

int urhgpu_pcm_to_iq_dev(urhgpu_ctx *ctx, const void *d_raw, int64_t n_frames, int channels, int sample_width, float *d_out) {
    if (!ctx || n_frames < 0 || (n_frames > 0 && (!d_raw || !d_out))) return URHGPU_ERR_ARG;
    if (channels < 1 || channels > 2 || sample_width < 1 || sample_width > 4) return URHGPU_ERR_ARG;      // (ValueError in the reference, :133, :164)
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_pcm_to_iq(d_raw, n_frames, channels, sample_width, d_out, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_fft_peak_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int64_t *peak_index) {
    if (!ctx || !peak_index || n < 1 || (n & (n - 1)) != 0 || !d_x) return URHGPU_ERR_ARG;
    int log2n = 0;
    while (((int64_t)1 << log2n) < n) ++log2n;
    if (log2n > 26) return URHGPU_ERR_UNSUPPORTED;           // (two LDS-sized factors of at most 8192 each)
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(ctx->arena.reserve(fft_peak_scratch_bytes(n) + 4096));
    ctx->arena.reset();
    void *scratch = ctx->arena.take(fft_peak_scratch_bytes(n));
    int64_t *d_peak = (int64_t *)ctx->arena.take(256);
    if (!scratch || !d_peak) return URHGPU_ERR_ARG;
    URH_TRY(launch_fft_peak((const float2 *)d_x, log2n, scratch, d_peak, ctx->stream));
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, peak_index, d_peak, 8));
    return URHGPU_OK;
}

// IQArray.export_to_sub's run lengths (IQArray.py:275-304), host arithmetic on the bytes convert_to(uint8) produced on the device: the
// reference walks the FIRST component of every sample with (lastvalue, counter) -- equal to lastvalue: counter += 1; different: when
// counter > 1 the run is appended (positive above 127, negative otherwise) and the new value starts a run of 1, when counter is 1
// NOTHING happens (the value is dropped and lastvalue stays: a single sample never ends a run); the last run is always appended.
int urhgpu_sub_encode_runs(const uint8_t *values, int64_t n, int64_t stride, int64_t *runs_out, int64_t cap, int64_t *n_runs) {
    if (!values || n <= 0 || stride < 1 || !n_runs || cap < 0 || (cap > 0 && !runs_out)) return URHGPU_ERR_ARG;     // (an empty array: NameError in the reference)
    int64_t k = 0, counter = 0;
    uint8_t last = values[0];
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t v = values[i * stride];
        if (v == last) { ++counter; continue; }
        if (counter > 1) {
            if (k < cap) runs_out[k] = last > 127 ? counter : -counter;
            ++k;
            counter = 1;
            last = v;
        }
    }
    if (k < cap) runs_out[k] = last > 127 ? counter : -counter;
    ++k;
    *n_runs = k;
    return k > cap ? URHGPU_ERR_CAPACITY : URHGPU_OK;
}

int urhgpu_path_minmax_dev(urhgpu_ctx *ctx, const void *d_samples, int dtype, int64_t start, int64_t end,
                           int64_t samples_per_pixel, void *d_values) {
    if (!ctx || !d_samples || !d_values || start < 0 || end <= start || samples_per_pixel < 1) return URHGPU_ERR_ARG;
    if (!value_bytes(dtype)) return URHGPU_ERR_DTYPE;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(launch_path_minmax(d_samples, dtype, start, end, samples_per_pixel, d_values, ctx->stream));
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_path_minmax(urhgpu_ctx *ctx, const void *samples, int dtype, int64_t n, int64_t start, int64_t end,
                       int64_t samples_per_pixel, void *values) {
    if (!ctx || !samples || !values || start < 0 || end <= start || end > n || samples_per_pixel < 1) return URHGPU_ERR_ARG;
    const int eb = value_bytes(dtype);
    if (!eb) return URHGPU_ERR_DTYPE;
    const int64_t pixels = (end - start + samples_per_pixel - 1) / samples_per_pixel;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(ctx->staging.reserve(align256((size_t)(end - start) * eb) + align256((size_t)pixels * 2 * eb) + 1024));
    ctx->staging.reset();
    void *d_in = nullptr;
    URH_TRY(stage_in(ctx, (const char *)samples + (size_t)start * eb, (size_t)(end - start) * eb, &d_in));
    void *d_val = ctx->staging.take((size_t)pixels * 2 * eb);
    if (!d_val) return URHGPU_ERR_ARG;
    URH_TRY(urhgpu_path_minmax_dev(ctx, d_in, dtype, 0, end - start, samples_per_pixel, d_val));
    URH_TRY(fetch_out(ctx, values, d_val, (size_t)pixels * 2 * eb));
    return URHGPU_OK;
}

}  // extern "C"
