// ctx.hip -- the context behind the C ABI of include/urhgpu.h: lifecycle, tuning, profiling, plain copies.
#include <chrono>

#include "pass.hpp"
#include "fdlibm_atan2f.h"
#include "glibc_sincosf.h"

namespace urh {

thread_local char g_hip_err[256] = "";
std::atomic<long long> g_center_host_syncs{0};
thread_local int g_center_scope = 0;
std::atomic<long long> g_noise_host_syncs{0};
thread_local int g_noise_scope = 0;
std::atomic<long long> g_records_host_syncs{0};
thread_local int g_records_scope = 0;

int Arena::reserve(size_t bytes) {
    if (bytes <= cap) return URHGPU_OK;
    if (base) { center_note_wait(); URH_HIP(hipFree(base)); base = nullptr; cap = 0; }      // (hipFree waits for the device)
    const size_t want = (bytes + (size_t(1) << 20)) & ~((size_t(1) << 20) - 1);
    URH_HIP(hipMalloc(&base, want));
    cap = want;
    used = 0;
    return URHGPU_OK;
}
void Arena::release() {
    if (base) { (void)hipFree(base); base = nullptr; cap = 0; used = 0; }
}

hipError_t wait_stream(const urhgpu_ctx *ctx, hipStream_t s) {
    center_note_wait();
    if (ctx->tune_spin_wait) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int it = 0;; ++it) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) return q;
            if ((it & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        }
    }
    return hipStreamSynchronize(s);
}
// pipelined mode: make the caller's stream wait for the tail of the last pass (no host blocking).  Every entry point that takes
// scratch from ctx->arena or launches on ctx->stream calls this first: on a pipelined context the arena is the one the last pass's
// tail may still be working in.
int join_tail(urhgpu_ctx *ctx) {
    if (ctx->tail_pending) {
        URH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_tail[(ctx->flip + 2) % 3], 0));       // the pass recorded last
        ctx->tail_pending = false;
    }
    return URHGPU_OK;
}

// CU mask of the hot stream on a 256-CU part: `removed` CUs of every XCD left out (see urhgpu_ctx_set_pipelined)
void hot_cu_mask(int removed, uint32_t mask[8]) {
    for (int w = 0; w < 8; ++w) mask[w] = 0;
    for (int i = 0; i < 256; ++i) {
        const int c = ((i % 8) - (i / 32) + 8) % 8, k = (i / 8) % 4;
        if (c * 4 + k >= removed) mask[i / 32] |= 1u << (i % 32);
    }
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_version(void) { return URHGPU_VERSION; }

const char *urhgpu_strerror(int status) {
    switch (status) {
        case URHGPU_OK: return "ok";
        case URHGPU_ERR_HIP: return "HIP runtime error";
        case URHGPU_ERR_DTYPE: return "Unsupported dtype";
        case URHGPU_ERR_ARG: return "bad argument";
        case URHGPU_ERR_CAPACITY: return "output capacity too small";
        case URHGPU_ERR_UNSUPPORTED: return "parameter outside the supported range";
        case URHGPU_ERR_NO_DEVICE: return "no usable GPU";
        default: return "unknown status";
    }
}

const char *urhgpu_last_hip_error(void) { return g_hip_err; }

int urhgpu_device_count(int *count) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return URHGPU_ERR_NO_DEVICE; }
    *count = c;
    return URHGPU_OK;
}

int urhgpu_ctx_create(int device, urhgpu_ctx **out) {
    if (!out) return URHGPU_ERR_ARG;
    int c = 0;
    if (urhgpu_device_count(&c) != URHGPU_OK || c <= 0 || device < 0 || device >= c) return URHGPU_ERR_NO_DEVICE;
    urhgpu_ctx *ctx = new (std::nothrow) urhgpu_ctx();
    if (!ctx) return URHGPU_ERR_ARG;
    ctx->device = device;
    URH_HIP(hipSetDevice(device));
    URH_HIP(hipGetDeviceProperties(&ctx->prop, device));
    URH_HIP(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    URH_HIP(hipMalloc((void **)&ctx->d_counts, 16 * sizeof(int64_t)));
    URH_HIP(hipMalloc((void **)&ctx->d_tickets, 16 * sizeof(int32_t)));     // [0..3] elections, [4..7] ResolveAux, [8..9] tile tail's huge-row counters
    URH_HIP(hipMemset(ctx->d_tickets, 0, 16 * sizeof(int32_t)));
    URH_HIP(hipMalloc(&ctx->d_noise_work, kNoiseWorkBytes));               // the noise chain's scratch: fixed, part of the context
    {   // d_tickets[4..7] is the ResolveAux block of the resolve kernels: kAuxNone x3, -1
        const int32_t aux0[4] = {kAuxNone, kAuxNone, kAuxNone, -1};
        URH_HIP(hipMemcpy(ctx->d_tickets + 4, aux0, sizeof(aux0), hipMemcpyHostToDevice));
    }
    URH_HIP(hipHostMalloc((void **)&ctx->h_counts, 32 * sizeof(int64_t)));
    memset(ctx->h_counts, 0, 32 * sizeof(int64_t));
    if (hipHostMalloc((void **)&ctx->h_small, kSmallPinned) != hipSuccess) { (void)hipGetLastError(); ctx->h_small = nullptr; }   // (optional: pageable copies work too)
    *out = ctx;
    return URHGPU_OK;
}

int urhgpu_ctx_destroy(urhgpu_ctx *ctx) {
    if (!ctx) return URHGPU_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->arena.release();
    ctx->staging.release();
    ctx->aux.release();
    ctx->fir_work.release();
    ctx->chunk_work.release();
    ctx->center_work.release();
    ctx->dc_work.release();
    ctx->batch_dc_mean.release();
    if (ctx->ev_dc) (void)hipEventDestroy(ctx->ev_dc);
    if (ctx->ev_center) (void)hipEventDestroy(ctx->ev_center);
    if (ctx->h_chunk) (void)hipHostFree(ctx->h_chunk);
    if (ctx->ev_fir) (void)hipEventDestroy(ctx->ev_fir);
    ctx->arena_alt.release();
    ctx->arena_alt2.release();
    if (ctx->hot_masked) { (void)hipStreamSynchronize(ctx->hot_masked); (void)hipStreamDestroy(ctx->hot_masked); }
    if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
    if (ctx->tail_stream) (void)hipStreamSynchronize(ctx->tail_stream);
    if (ctx->own_tail_stream && ctx->tail_stream) (void)hipStreamDestroy(ctx->tail_stream);
    if (ctx->d_seg) {
        (void)hipFree(ctx->d_seg);
        if (ctx->bits_stream) { (void)hipStreamSynchronize(ctx->bits_stream); (void)hipStreamDestroy(ctx->bits_stream); }
        for (hipEvent_t e : ctx->ev_piece) if (e) (void)hipEventDestroy(e);
        for (int k = 0; k < 3; ++k) {
            if (ctx->ev_hot_done[k]) (void)hipEventDestroy(ctx->ev_hot_done[k]);
            if (ctx->ev_bits[k]) (void)hipEventDestroy(ctx->ev_bits[k]);
            for (hipEvent_t e : ctx->ev_rows[k]) if (e) (void)hipEventDestroy(e);
        }
    }
    if (ctx->ev_hot) { (void)hipEventDestroy(ctx->ev_hot); (void)hipEventDestroy(ctx->ev_tail[0]); (void)hipEventDestroy(ctx->ev_tail[1]); (void)hipEventDestroy(ctx->ev_tail[2]); }
    free_shard_session(ctx);
    for (hipEvent_t e : ctx->prof_events) (void)hipEventDestroy(e);
    if (ctx->d_counts) (void)hipFree(ctx->d_counts);
    if (ctx->d_tickets) (void)hipFree(ctx->d_tickets);
    if (ctx->d_noise_work) (void)hipFree(ctx->d_noise_work);
    if (ctx->d_desc) (void)hipFree(ctx->d_desc);
    if (ctx->d_rdesc) (void)hipFree(ctx->d_rdesc);
    if (ctx->h_counts) (void)hipHostFree(ctx->h_counts);
    if (ctx->h_small) (void)hipHostFree(ctx->h_small);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return URHGPU_OK;
}

int urhgpu_ctx_set_stream(urhgpu_ctx *ctx, void *hip_stream) {
    if (!ctx) return URHGPU_ERR_ARG;
    ctx->stream = (hipStream_t)hip_stream;
    return URHGPU_OK;
}

int urhgpu_ctx_use_private_stream(urhgpu_ctx *ctx) {
    if (!ctx) return URHGPU_ERR_ARG;
    ctx->stream = ctx->own_stream;
    return URHGPU_OK;
}

int urhgpu_ctx_sync(urhgpu_ctx *ctx) {
    if (!ctx) return URHGPU_ERR_ARG;
    if (ctx->hot_masked) URH_HIP(hipStreamSynchronize(ctx->hot_masked));
    if (ctx->bits_stream) URH_HIP(hipStreamSynchronize(ctx->bits_stream));
    if (ctx->tail_stream) URH_HIP(hipStreamSynchronize(ctx->tail_stream));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    ctx->tail_pending = false;
    return URHGPU_OK;
}

int urhgpu_ctx_set_pipelined(urhgpu_ctx *ctx, int enable, void *tail_stream) {
    if (!ctx) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    if (ctx->own_tail_stream && ctx->tail_stream) { (void)hipStreamDestroy(ctx->tail_stream); }
    ctx->tail_stream = nullptr; ctx->own_tail_stream = false; ctx->pipelined = false;
    if (ctx->hot_masked) { (void)hipStreamSynchronize(ctx->hot_masked); (void)hipStreamDestroy(ctx->hot_masked); ctx->hot_masked = nullptr; }
    if (!enable) return URHGPU_OK;
    if (tail_stream) ctx->tail_stream = (hipStream_t)tail_stream;
    else {
        URH_HIP(hipStreamCreateWithFlags(&ctx->tail_stream, hipStreamNonBlocking));
        ctx->own_tail_stream = true;
    }
    if (!ctx->ev_hot) {
        URH_HIP(hipEventCreateWithFlags(&ctx->ev_hot, hipEventDisableTiming));
        for (hipEvent_t &e : ctx->ev_tail) URH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // The hot kernel of a pipelined pass runs on a private stream whose CU mask leaves hot_cus_removed CUs per XCD out (default 4: 224 of
    // the 256 CUs).  Measured (round 3, profiles/HISTORY.md): the kernel -- and a pure copy of its shape -- is FASTEST there: 0.2666 ms
    // = 6.04 TB/s on 224 CUs against 0.2799 ms = 5.75 TB/s on all 256 (248 / 240 / 232 CUs: 0.2746 / 0.2718 / 0.2708; 208 / 192: 0.2746 /
    // 0.2752; 160: 0.311): 256 CUs of streaming wavefronts ask more of the HBM than it serves well.  And the 32 CUs it leaves alone are
    // where the previous pass's tail, the blob packing and the collectives of sharded passes find their wave slots at once.  The mask
    // bits of the removed CUs are chosen so that every XCD loses the same number whichever way bits map to XCDs (bit i -> XCD i / 32 or
    // i % 8): class (i % 8 - i / 32) mod 8 and slot (i / 8) % 4 enumerate 32 sets of 8 CUs, one per XCD each.
    if (ctx->tune_hot_cus_removed > 0 && ctx->prop.multiProcessorCount == 256) {
        const int words = 8;
        uint32_t mask[8];
        hot_cu_mask(ctx->tune_hot_cus_removed, mask);
        // (a runtime that cannot make the masked stream is no reason to fail: the hot kernel then runs on the caller's stream as before)
        if (hipExtStreamCreateWithCUMask(&ctx->hot_masked, (uint32_t)words, mask) != hipSuccess) { (void)hipGetLastError(); ctx->hot_masked = nullptr; }
        if (ctx->hot_masked && !ctx->ev_in && hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamDestroy(ctx->hot_masked);
            ctx->hot_masked = nullptr;
        }
    }
    ctx->pipelined = true;
    return URHGPU_OK;
}

// Tuning values of the pipelined mode (defaults = what is measured and shipped; the A/B tool tools/ab.sh sets others through bench.py's
// URH_TUNE_* environment, read THERE -- the library itself reads no environment variable).  The knobs earlier rounds measured as useless
// are gone; their records are in profiles/HISTORY.md.
//   hot_lds_kb               dynamic LDS per hot workgroup in KiB (fewer of them per CU: room for the previous pass's tail); default 0
//   hot_lds_kb_sharded       the same for the urhgpu_shard_* passes that keep the generic tail (ASK); default 33
//   hot_cus_removed_per_xcd  CUs per XCD the hot kernel of a pipelined pass leaves alone (before urhgpu_ctx_set_pipelined); default 4, 0: no mask
//   profile_bracket          1: urhgpu_ctx_profile_* report the stream-level bracket around the hot launch instead of the dispatch's own timing
//   stream_policy            which tail a pass of urhgpu_stream_* takes (common.hpp: tune_stream_policy); default 5
//   stream_segments          rows segments of a segmented pass; default 7
//   stream_latency           1: a pass that finds the pipeline idle runs its tail in segments (lowest latency for ONE capture); default 0
//   stream_pos_direct        1 (default): direct passes ship bit_sample_pos themselves
//   upload_pieces            pieces of urhgpu_stream_push_upload; default 4
//   spin_wait                1 (default): the estimator calls poll their stream for the few hundred microseconds they wait (wait_stream)
//   wide_int                 1: passes over SIGNED INTEGER FSK captures take the hot kernel's instantiation with the wide loop (captures whose phase
//                            steps leave the fast loop's window, DESIGN 4: a quarter faster there, 5 % slower on narrow ones).  Capture streams
//                            decide by themselves (k_wide_probe); one-shot and sharded passes have no probe to go by: this key is the caller's word.  default 0
//   costas_dev_rounds        who drives the re-speculation rounds of the parallel Costas loop (costas.hip).  -1 (default): the host for one-shot passes on
//                            a context that is not pipelined (it synchronises the stream once per round), the device inside capture streams and on
//                            pipelined contexts, with as many rounds queued as the capture's chunk count affords (costas_auto_rounds).  0 .. 24: the
//                            device everywhere, with exactly that many re-speculation rounds queued; what they leave is walked serially by the stitch
//   auto_center_max_bins     bins the histogram pool of the automatic center (urhgpu_detect_center_dev, urhgpu_iq_to_bits_auto_center_dev) holds
//                            for its one range; a histogram with more comes back as flag 2.  default 4096 (what k_me_hist keeps in LDS)
//   shard_summary_generic    1: the local pass of urhgpu_shard_runs_dev as the three generic resolve launches instead of k_shard_summary; default 0
int urhgpu_ctx_set_tuning(urhgpu_ctx *ctx, const char *key, int value) {
    if (!ctx || !key) return URHGPU_ERR_ARG;
    if (!strcmp(key, "hot_lds_kb")) { if (value < 0 || value > 150) return URHGPU_ERR_ARG; ctx->hot_lds_pad = value * 1024; }
    else if (!strcmp(key, "hot_lds_kb_sharded")) { if (value < 0 || value > 150) return URHGPU_ERR_ARG; ctx->hot_lds_pad_sharded = value * 1024; }
    else if (!strcmp(key, "profile_bracket")) ctx->prof_bracket = value != 0;
    else if (!strcmp(key, "hot_cus_removed_per_xcd")) { if (value < 0 || value > 16) return URHGPU_ERR_ARG; ctx->tune_hot_cus_removed = value; }
    else if (!strcmp(key, "stream_segments")) { if (value < 1 || value > kMaxSegments) return URHGPU_ERR_ARG; ctx->tune_stream_segments = value; }
    else if (!strcmp(key, "stream_policy")) { if (value < 0 || value > 6) return URHGPU_ERR_ARG; ctx->tune_stream_policy = value; }
    else if (!strcmp(key, "stream_latency")) { ctx->tune_stream_latency = value != 0; }
    else if (!strcmp(key, "stream_pos_direct")) { ctx->tune_stream_pos_direct = value != 0; }
    else if (!strcmp(key, "spin_wait")) { ctx->tune_spin_wait = value != 0; }
    else if (!strcmp(key, "shard_summary_generic")) { ctx->tune_shard_summary_generic = value != 0; }
    else if (!strcmp(key, "wide_int")) { ctx->tune_wide_int = value != 0; }
    else if (!strcmp(key, "costas_dev_rounds")) { if (value < -1 || value > 24) return URHGPU_ERR_ARG; ctx->tune_costas_dev_rounds = value; }
    else if (!strcmp(key, "upload_pieces")) { if (value < 2 || value > kMaxSegments) return URHGPU_ERR_ARG; ctx->tune_upload_pieces = value; }
    else if (!strcmp(key, "auto_center_max_bins")) { if (value < 1 || value > (1 << 20)) return URHGPU_ERR_ARG; ctx->tune_center_max_bins = value; }
    else return URHGPU_ERR_ARG;
    return URHGPU_OK;
}

int urhgpu_ctx_join(urhgpu_ctx *ctx) {
    if (!ctx) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    return join_tail(ctx);
}

// Does this host's libm evaluate sinf / cosf / atan2f the way the device code restates them?  The reference's Costas loop and FSK
// demodulation call the HOST's libm (signal_functions.pyx:252-330, :375, compiled as C++: sinf / cosf / atan2f), which is not correctly
// rounded: x86-64 glibc picks an FMA or a non-FMA build of sinf / cosf at run time, and the two differ on about one float in 10^9.  The
// device code restates the FMA build (glibc_sincosf.h, URH_SINCOSF_FMA = 1).  Checked: the 17 arguments below |x| = 120 on which the two
// builds differ (tools/libm_probe/scan.c finds them: an exhaustive scan), both signs, plus pseudo-random arguments; atan2f (one build
// in glibc) on pseudo-random operand pairs of every quadrant.  out4 = {sinf / cosf results compared, mismatches, atan2f results
// compared, mismatches}.  A mismatch means: on THIS host the reference itself would produce other bits than on the hosts the parity
// tests ran on, and the GPU's PSK / FSK output follows those, not this host's reference.  Host arithmetic only; no GPU needed.
int urhgpu_host_libm_check(int64_t *out4) {
    if (!out4) return URHGPU_ERR_ARG;
    static const uint32_t kDiscriminating[17] = {0x418a3adbu, 0x418a3adcu, 0x418a3addu, 0x418a3adeu, 0x41bc76d9u, 0x4202eb4bu, 0x4255b0a9u, 0x4280ce28u,
                                                 0x42687a55u, 0x42a35c07u, 0x42a35d44u, 0x42870e40u, 0x42a97360u, 0x42c55faau, 0x42d8d23eu, 0x42e87a55u,
                                                 0x42cf5854u};
    int64_t n_sc = 0, bad_sc = 0, n_at = 0, bad_at = 0;
    auto same = [](float a, float b) { uint32_t x, y; memcpy(&x, &a, 4); memcpy(&y, &b, 4); return x == y || (a != a && b != b); };
    auto check_sc = [&](float x) {
        volatile float vx = x;                                   // (keep the compiler from folding the libm calls)
        n_sc += 2;
        if (!same(sinf(vx), urh_sinf(x))) ++bad_sc;
        if (!same(cosf(vx), urh_cosf(x))) ++bad_sc;
    };
    for (uint32_t u : kDiscriminating) {
        float x; memcpy(&x, &u, 4);
        check_sc(x); check_sc(-x);
    }
    uint64_t s = 0x243f6a8885a308d3ull;
    auto next = [&]() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); };
    for (int i = 0; i < 4096; ++i) {
        const uint64_t z = next();
        check_sc((float)((double)(int64_t)(z >> 11) * (1.0 / 9007199254740992.0) * 240.0 - 120.0));      // uniform in (-120, 120)
        const uint32_t a = (uint32_t)z, b = (uint32_t)(z >> 32);
        // operands of every sign and of magnitudes 2^-20 .. 2^20
        float y, x;
        const uint32_t uy = (a & 0x807fffffu) | (((a >> 23) % 41u + 107u) << 23), ux = (b & 0x807fffffu) | (((b >> 23) % 41u + 107u) << 23);
        memcpy(&y, &uy, 4); memcpy(&x, &ux, 4);
        volatile float vy = y, vx = x;
        ++n_at;
        if (!same(atan2f(vy, vx), urh_atan2f(y, x))) ++bad_at;
    }
    out4[0] = n_sc; out4[1] = bad_sc; out4[2] = n_at; out4[3] = bad_at;
    return URHGPU_OK;
}

int urhgpu_ctx_info(urhgpu_ctx *ctx, int *compute_units, int *wavefront, int64_t *hbm_bytes, char *name, int name_cap) {
    if (!ctx) return URHGPU_ERR_ARG;
    if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
    if (wavefront) *wavefront = ctx->prop.warpSize;
    if (hbm_bytes) *hbm_bytes = (int64_t)ctx->prop.totalGlobalMem;
    if (name && name_cap > 0) { strncpy(name, ctx->prop.name, (size_t)name_cap - 1); name[name_cap - 1] = 0; }
    return URHGPU_OK;
}

int urhgpu_ctx_reserve(urhgpu_ctx *ctx, int64_t n_samples, int tolerance) {
    if (!ctx || n_samples < 0 || tolerance < 0) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    const Plan pl = make_plan(ctx, n_samples, tolerance);
    const int64_t cap_rows = n_samples / ((int64_t)tolerance + 1) + 2;
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, cap_rows, true, true)));
    if (ctx->pipelined) {
        URH_TRY(ctx->arena_alt.reserve(digitize_scratch_bytes(pl, cap_rows, true, true)));
        URH_TRY(ctx->arena_alt2.reserve(digitize_scratch_bytes(pl, cap_rows, true, true)));
    }
    return URHGPU_OK;
}

int urhgpu_ctx_profile_begin(urhgpu_ctx *ctx, int max_records) {
    if (!ctx || max_records < 0) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    while ((int)ctx->prof_events.size() < 4 * max_records) {
        hipEvent_t e;
        URH_HIP(hipEventCreate(&e));
        ctx->prof_events.push_back(e);
    }
    ctx->prof_used = 0;
    ctx->prof_on = max_records > 0;
    return URHGPU_OK;
}

int urhgpu_ctx_profile_end(urhgpu_ctx *ctx, float *ms_out, int cap, int *n_records) {
    if (!ctx || !n_records) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    if (ctx->hot_masked) URH_HIP(hipStreamSynchronize(ctx->hot_masked));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    ctx->prof_on = false;
    const int n = ctx->prof_used;
    *n_records = n;
    const bool bracket = ctx->prof_bracket;                          // report the stream-level bracket instead (comparison)
    for (int k = 0; k < n && k < cap; ++k) {
        const int base = 4 * k + ((ctx->prof_dispatch[(size_t)k] && !bracket) ? 2 : 0);
        URH_HIP(hipEventElapsedTime(&ms_out[k], ctx->prof_events[base], ctx->prof_events[base + 1]));
    }
    return URHGPU_OK;
}

int urhgpu_ctx_costas_stats(urhgpu_ctx *ctx, int32_t *out4) {
    if (!ctx || !out4) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    const int32_t *h = (const int32_t *)(ctx->h_counts + 12);
    out4[0] = h[0]; out4[1] = h[1]; out4[2] = h[2]; out4[3] = h[4];
    return URHGPU_OK;
}

int urhgpu_ctx_costas_stats5(urhgpu_ctx *ctx, int32_t *out5) {
    if (!ctx || !out5) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    memcpy(out5, ctx->h_counts + 12, 20);
    return URHGPU_OK;
}

int urhgpu_memcpy_to_host(urhgpu_ctx *ctx, const void *d_src, void *host_dst, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!d_src || !host_dst))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    if (bytes) URH_HIP(hipMemcpy(host_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return URHGPU_OK;
}

int urhgpu_memcpy_dtod(urhgpu_ctx *ctx, void *d_dst, const void *d_src, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!d_src || !d_dst))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    if (bytes) URH_HIP(hipMemcpy(d_dst, d_src, (size_t)bytes, hipMemcpyDeviceToDevice));
    return URHGPU_OK;
}

}  // extern "C"
