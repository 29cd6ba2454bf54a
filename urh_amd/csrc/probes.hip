// probes.hip -- measurement and test hooks (urhgpu_test_*, urhgpu_bench_*): nothing the product's paths call.
#include "pass.hpp"

using namespace urh;

#define URH_PROBE_WPB 4     // wavefronts per chunk of the complex64 FSK bit-plane kernel (demod_runs.hip: URH_WPB)

namespace urh {
bool g_tile_tail = true;           // test hook (urhgpu_test_force_generic_tail): 0 routes single-GPU non-ASK captures through the generic 8-launch tail as well
int g_force_tiles_per_chunk = 0;   // test hook (urhgpu_test_force_tiles_per_chunk): 0 = make_plan's size-dependent choice, 1..4 = that many tiles per chunk
}

extern "C" {

int urhgpu_test_fast_division_dev(urhgpu_ctx *ctx, uint64_t seed, int reps, uint64_t *n_mismatch) {
    if (!ctx || !n_mismatch || reps < 0) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemsetAsync(ctx->d_counts, 0, 8, ctx->stream));
    launch_test_div(seed, reps, (unsigned long long *)ctx->d_counts, ctx->stream);
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, ctx->h_counts, ctx->d_counts, 8));
    *n_mismatch = (uint64_t)ctx->h_counts[0];
    return URHGPU_OK;
}

int urhgpu_test_force_merge_ambiguous(int on) {
    const int was = urh::g_force_merge_ambiguous ? 1 : 0;
    urh::g_force_merge_ambiguous = on != 0;
    return was;
}

int urhgpu_test_sincosf_fast_dev(urhgpu_ctx *ctx, uint64_t *n_mismatch) {
    if (!ctx || !n_mismatch) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemsetAsync(ctx->d_counts, 0, 8, ctx->stream));
    launch_test_sincosf_fast((unsigned long long *)ctx->d_counts, ctx->stream);
    URH_HIP(hipGetLastError());
    URH_TRY(fetch_out(ctx, ctx->h_counts, ctx->d_counts, 8));
    *n_mismatch = (uint64_t)ctx->h_counts[0];
    return URHGPU_OK;
}

int urhgpu_bench_copy_ceiling_dev(urhgpu_ctx *ctx, const float *d_in, float *d_out, int64_t n_samples, int shape, int reps, float *ms_per_copy) {
    if (!ctx || !d_in || !d_out || !ms_per_copy || n_samples < 8192 || n_samples % 8192 || reps < 1 || shape < 0 || shape > 2) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    hipStream_t cs = ctx->stream;
    if (shape == 2) {                                      // shape 0 on the CUs the hot kernel of pipelined passes runs on
        if (!ctx->hot_masked) return URHGPU_ERR_UNSUPPORTED;
        cs = ctx->hot_masked; shape = 0;
    }
    hipEvent_t e0, e1;
    URH_HIP(hipEventCreate(&e0));
    URH_HIP(hipEventCreate(&e1));
    for (int k = 0; k < 3; ++k) launch_copy_shape(d_in, d_out, n_samples, shape, cs);
    URH_HIP(hipEventRecord(e0, cs));
    for (int k = 0; k < reps; ++k) launch_copy_shape(d_in, d_out, n_samples, shape, cs);
    URH_HIP(hipEventRecord(e1, cs));
    URH_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    URH_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_per_copy = ms / (float)reps;
    return URHGPU_OK;
}

// Probe (tools/boundary_probe.py; profiles/r05_boundary_anatomy.txt): `launches` back-to-back launches of the hot kernel ALONE (complex64
// 2-FSK, qad written, no tail) on one stream, every wavefront 0 leaving its s_memrealtime stamps in its ChunkInfo.
// synthetic company for the hot kernel (urhgpu_test_hot_probe: load_kind): dependent integer / float arithmetic for `ticks` x 10 ns ...
__global__ void k_probe_valu(long long ticks, int prio, float *sink) {
    if (prio) __builtin_amdgcn_s_setprio(3);
    const long long t0 = (long long)wall_clock64();
    float x = (float)threadIdx.x, y = 1.0f;
    unsigned long long z = threadIdx.x;
    do {
#pragma unroll
        for (int k = 0; k < 64; ++k) { x = x * 1.0001f + y; y = y * 0.9999f + x; z = z * 6364136223846793005ull + 1442695040888963407ull; }
    } while ((long long)wall_clock64() - t0 < ticks);
    if (x == 12345.678f && z == 42) *sink = y;
}
// ... or dependent random 64-byte-line loads over `lines` lines of `mem`
__global__ void k_probe_latency(long long ticks, const unsigned long long *mem, unsigned long long lines, unsigned long long *sink) {
    const long long t0 = (long long)wall_clock64();
    unsigned long long at = (blockIdx.x * 256ull + threadIdx.x) * 0x9e3779b97f4a7c15ull, acc = 0;
    do {
#pragma unroll 1
        for (int k = 0; k < 8; ++k) { const unsigned long long v = mem[(at % lines) * 8]; acc += v; at = at * 6364136223846793005ull + v + 1442695040888963407ull; }
    } while ((long long)wall_clock64() - t0 < ticks);
    if (acc == 0x1234567ull) *sink = acc;
}

__global__ void k_probe_spin(long long ticks) {              // one wavefront that does nothing for `ticks` x 10 ns (a bubble between two hot kernels)
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}

int urhgpu_test_hot_stamps(int on) { urh::g_stamp_probe = (on != 0); return URHGPU_OK; }
int urhgpu_test_tail_skip(int mask) { urh::g_tail_skip = mask; return URHGPU_OK; }

// the chunk tables of the three most recent pipelined passes (current, previous, the one before), n_chunks entries each -- the table is
// the first thing a pass takes from its scratch arena
int urhgpu_test_fetch_chunk_tables(urhgpu_ctx *ctx, void *host_dst, int64_t n_chunks) {
    if (!ctx || !host_dst || n_chunks < 1) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(urhgpu_ctx_sync(ctx));
    const size_t bytes = (size_t)n_chunks * sizeof(ChunkInfo);
    const urh::Arena *order[3] = {&ctx->arena, &ctx->arena_alt2, &ctx->arena_alt};
    for (int k = 0; k < 3; ++k) {
        if (!order[k]->base || order[k]->cap < bytes) { memset((char *)host_dst + k * bytes, 0, bytes); continue; }
        URH_HIP(hipMemcpy((char *)host_dst + k * bytes, order[k]->base, bytes, hipMemcpyDeviceToHost));
    }
    return URHGPU_OK;
}

int urhgpu_test_hot_probe(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad, int stream_kind, int event_mode,
                          int graded, int launches, int keep, void *d_chunks_out, int64_t *n_chunks_out, float *dur_ms, float *gap_ms, int bubble_us,
                          int load_kind) {
    if (!ctx || !d_iq || !p || !d_qad || !d_chunks_out || !n_chunks_out || launches < 1 || keep < 1 || keep > launches || n < kTile || n % kTile) return URHGPU_ERR_ARG;
    if (p->dtype != URHGPU_DT_F32 || p->mod != URHGPU_MOD_FSK || p->bits_per_symbol != 1) return URHGPU_ERR_UNSUPPORTED;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    URH_TRY(urhgpu_ctx_sync(ctx));
    const Plan pl = make_plan(ctx, n, p->tolerance);
    const int64_t g = std::min<int64_t>(std::max(graded, 0), pl.n_chunks);
    const int64_t short_len = pl.chunk_len / 4;
    if (g > 0 && ((short_len % (URH_PROBE_WPB * kRowSamples)) != 0 || n % pl.chunk_len != 0)) return URHGPU_ERR_UNSUPPORTED;
    const int64_t n_launch = pl.n_chunks + 3 * g;              // the last g chunks cut into four short ones each
    URH_TRY(ctx->arena.reserve((size_t)n_launch * sizeof(ChunkInfo) + (size_t)n_launch * pl.slab_stride * 8 + 4096));
    ctx->arena.reset();
    ChunkInfo *chunks = (ChunkInfo *)ctx->arena.take((size_t)n_launch * sizeof(ChunkInfo));
    uint64_t *slab = (uint64_t *)ctx->arena.take((size_t)n_launch * pl.slab_stride * 8);
    if (!chunks || !slab) return URHGPU_ERR_ARG;
    RunArgs a;
    URH_TRY(hot_run_args(ctx, p, pl, n, 0, true, &a));
    a.in = d_iq; a.qad = d_qad; a.wide_int = 0;               // (complex64 only: no wide loop whatever the context's word)
    a.chunks = chunks; a.slab = slab; a.stamp_probe = 1;
    if (g > 0) { a.graded_from = pl.n_chunks - g; a.graded_len = short_len; }
    hipStream_t s = ctx->stream;
    if (stream_kind == 1) { if (!ctx->hot_masked) return URHGPU_ERR_UNSUPPORTED; s = ctx->hot_masked; }
    // event_mode 0: plain launches; 1: a completion event (timing disabled) attached to every dispatch, as the product's pipelined passes
    // do; 2: the same, created with hipEventDisableSystemFence | hipEventReleaseToDevice; 3: timing events (start + stop) on every dispatch
    std::vector<hipEvent_t> ev((size_t)launches * 2, nullptr);
    if (event_mode != 0) {
        const unsigned fl = event_mode == 1 ? hipEventDisableTiming : event_mode == 2 ? (hipEventDisableTiming | hipEventDisableSystemFence | hipEventReleaseToDevice) : hipEventDefault;
        for (auto &e : ev) URH_HIP(hipEventCreateWithFlags(&e, fl));
    }
    // load_kind: synthetic company on a second stream, started behind hot kernel j's completion event (so it runs beside hot kernel j + 1, as
    // the product's tail does).  1: 256 wavefronts of arithmetic for 200 us on the CUs the hot mask leaves out; 2: the same at s_setprio 3;
    // 3: 4096 workgroups of 4 wavefronts, 4 us of arithmetic each at s_setprio 3, anywhere on the chip; 4: 256 wavefronts of dependent random
    // loads for 200 us on the CUs left out; 5: six empty one-wavefront kernels in a row (kernel boundaries: cache write-back / invalidate)
    hipStream_t s2 = nullptr;
    void *load_mem = nullptr;
    if (load_kind != 0) {
        if (event_mode == 0 || event_mode == 3) return URHGPU_ERR_ARG;
        if (load_kind == 3 || load_kind == 5) URH_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        else {
            uint32_t m[8], inv[8];
            hot_cu_mask(ctx->tune_hot_cus_removed, m);
            for (int w = 0; w < 8; ++w) inv[w] = ~m[w];
            URH_HIP(hipExtStreamCreateWithCUMask(&s2, 8, inv));
        }
        URH_HIP(hipMalloc(&load_mem, size_t(256) << 20));
        URH_HIP(hipMemset(load_mem, 1, size_t(256) << 20));
        URH_HIP(hipDeviceSynchronize());
    }
    for (int j = 0; j < launches; ++j) {
        // the last `keep` launches write their chunk tables straight into the caller's buffer (nothing between two hot kernels)
        a.chunks = (j >= launches - keep) ? (ChunkInfo *)d_chunks_out + (size_t)(j - (launches - keep)) * n_launch : chunks;
        HotEvents he;
        if (event_mode != 0) { he.start = event_mode == 3 ? ev[2 * j] : nullptr; he.stop = ev[2 * j + 1]; }
        URH_TRY(launch_demod_runs_iq(a, p->dtype, p->mod, true, s, &he));
        if (bubble_us > 0) hipLaunchKernelGGL(k_probe_spin, dim3(1), dim3(64), 0, s, (long long)bubble_us * 100);
        if (load_kind != 0) {
            URH_HIP(hipStreamWaitEvent(s2, ev[2 * j + 1], 0));
            if (load_kind == 1 || load_kind == 2) hipLaunchKernelGGL(k_probe_valu, dim3(64), dim3(256), 0, s2, 20000ll, load_kind == 2 ? 1 : 0, (float *)load_mem);
            else if (load_kind == 3) hipLaunchKernelGGL(k_probe_valu, dim3(4096), dim3(256), 0, s2, 400ll, 1, (float *)load_mem);
            else if (load_kind == 4) hipLaunchKernelGGL(k_probe_latency, dim3(64), dim3(256), 0, s2, 20000ll, (const unsigned long long *)load_mem, (unsigned long long)((size_t(256) << 20) / 64), (unsigned long long *)load_mem);
            else for (int k = 0; k < 6; ++k) hipLaunchKernelGGL(k_probe_spin, dim3(1), dim3(64), 0, s2, 100ll);
        }
    }
    URH_HIP(hipStreamSynchronize(s));
    if (s2) { URH_HIP(hipStreamSynchronize(s2)); (void)hipStreamDestroy(s2); (void)hipFree(load_mem); }
    if (event_mode == 3 && dur_ms && gap_ms) {
        for (int j = 0; j < launches; ++j) {
            URH_HIP(hipEventElapsedTime(&dur_ms[j], ev[2 * j], ev[2 * j + 1]));
            if (j + 1 < launches) URH_HIP(hipEventElapsedTime(&gap_ms[j], ev[2 * j + 1], ev[2 * j + 2]));
        }
    }
    for (auto e : ev) if (e) (void)hipEventDestroy(e);
    *n_chunks_out = n_launch;
    return URHGPU_OK;
}

int urhgpu_test_force_state_bytes(int on) { urh::g_force_state_bytes = (on != 0); return URHGPU_OK; }
int urhgpu_test_force_generic_tail(int on) { urh::g_tile_tail = (on == 0); return URHGPU_OK; }
int64_t urhgpu_test_wide_int_launches(void) { return (int64_t)urh::g_wide_int_launches.load(); }
int64_t urhgpu_test_costas_host_syncs(void) { return (int64_t)urh::g_costas_host_syncs.load(); }
int urhgpu_test_costas_scratch(int64_t n, int loop_order, int64_t *out3) {
    if (!out3 || n < 0 || (loop_order != 2 && loop_order != 4)) return URHGPU_ERR_ARG;
    urh::costas_scratch_layout(n, loop_order == 4 ? 8 : 4, out3);
    return URHGPU_OK;
}

int urhgpu_test_force_tiles_per_chunk(int tiles) {
    if (tiles < 0 || tiles > 4) return URHGPU_ERR_ARG;
    urh::g_force_tiles_per_chunk = tiles;
    return URHGPU_OK;
}

int urhgpu_test_atan2f_dev(urhgpu_ctx *ctx, const float *d_y, const float *d_x, int64_t n, float *d_out) {
    if (!ctx) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    launch_test_atan2f(d_y, d_x, n, d_out, ctx->stream);
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // extern "C"
