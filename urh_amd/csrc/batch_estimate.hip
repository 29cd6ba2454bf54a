// batch_estimate.hip -- the message ranges of a batch of captures (include/urhgpu.h "a batch of captures: message ranges per capture").
//
// The estimate of a capture starts with its message ranges (AutoInterpretation.estimate, AutoInterpretation.py:373-470:
// segment_messages_from_magnitudes on the magnitudes).  For one capture that is the hot kernel's seg_mode and msg_ranges.hip -- a pass per
// capture.  Here K captures lie back to back in one buffer, as in batch.hip, and three launches give the ranges of all of them:
//   k_batch_segments<DT>   a WAVEFRONT PER CAPTURE, in the plan's order (longest first).  A step is kBatchSegStep consecutive samples, one
//                          per lane; every lane evaluates seg_above<DT> (seg_above.hpp: the comparison msg_ranges.hip makes) with the
//                          capture's OWN threshold; ballot gives the step's above-noise mask, and wave-uniform code follows
//                          auto_interpretation.pyx:55-111 over the RUNS of set and clear bits of that mask (find-first-set on the mask and on
//                          its complement), not sample by sample.  conseq_above / conseq_below live across steps, so a run that reaches the
//                          outlier tolerance switches the state at its tenth sample wherever the step seam falls.
//   k_batch_seg_scan       one workgroup: dir[c] = segments stored for the captures before c, dir[k] = M
//   k_batch_seg_pack       a bounded grid of wavefronts striding over the captures: capture c's pairs to out[dir[c] ..)
// Nothing waits for another wavefront or uses an atomic.  A wavefront's state is a handful of scalars; its only stores are lane 0's pairs
// into the capture's own region (bounded by its capacity) and the capture's count.  No load leaves [start[c], start[c + 1]).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"

// seg_above<F32> takes the magnitude's square root with __builtin_sqrtf, which the compiler expands into two v_fma_f32.  In this file the
// root is taken in fp64 and rounded once to fp32 -- for an fp32 operand that IS the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits: the
// second rounding is innocuous; batch_kernels.hpp's URH_FSQRT is the same form) --, so that an fp32 FMA in this file's assembly could only
// be v.x * v.x + v.y * v.y contracted into one rounding, which tests/test_batch_estimate_host.py then looks for.  seg_above.hpp's text stays
// as msg_ranges.hip compiles it; the headers it includes are included above, so the name is replaced in its own text alone.
__device__ __forceinline__ float batch_seg_sqrtf(float x) {
    double dx = x;
#if defined(__HIP_DEVICE_COMPILE__)
    __asm__ volatile("" : "+v"(dx));      // (keeps the optimiser from folding the form back into the fp32 root)
#endif
    return (float)__builtin_sqrt(dx);
}
#define __builtin_sqrtf(x) batch_seg_sqrtf(x)
#include "seg_above.hpp"
#undef __builtin_sqrtf

namespace urh {

constexpr int kBatchSegStep = 64;              // samples per step: one per lane
constexpr int64_t kSegOutlierTolerance = 10;   // outlier_tolerance (:72)
constexpr int kSegPackGrid = 1024;             // k_batch_seg_pack: at most this many wavefronts, striding over the captures

struct BatchSegArgs {
    const void *iq;            // K captures back to back, (total, 2) of the dtype
    const int64_t *start;      // [k + 1] first sample of each capture
    const int64_t *plan;       // [3 k] urhgpu_batch_plan's: only the launch order, plan[2 k ..), is read
    const float *thr;          // [k] noise threshold of each capture
    const int64_t *region;     // [k] first pair of each capture's region in seg
    int64_t k, total;
    int64_t *seg;              // [cap_seg][2]
    int64_t cap_seg;
    int64_t *counts;           // [k] segments of each capture (exact, whatever was stored)
    int64_t *dir;              // [k + 1]
    int64_t *out;              // [cap_out][2] the stored segments of all captures, compacted in capture order
    int64_t cap_out;
};

// what capture c may use: its samples, checked against the buffer, and its region of n / 20 + 1 pairs, checked against seg
struct BatchSegCapture { int64_t s0, n, roff, cap; };
__device__ __forceinline__ BatchSegCapture batch_seg_capture(const BatchSegArgs &b, int64_t c) {
    BatchSegCapture v;
    v.s0 = b.start[c];
    const int64_t s1 = b.start[c + 1];
    const bool ok = v.s0 >= 0 && s1 >= v.s0 && s1 <= b.total && s1 - v.s0 <= 0x7fffffffll;
    v.n = ok ? s1 - v.s0 : 0;                              // a refused start or end: nothing is read
    v.roff = b.region[c];
    v.cap = v.n / (2 * kSegOutlierTolerance) + 1;          // ten samples to open a segment and ten to close it
    if (!ok || v.roff < 0 || v.roff > b.cap_seg || v.cap > b.cap_seg - v.roff) v.cap = 0;      // no region: nothing is stored, the count still is
    return v;
}

// the raw sample of a type, as seg_above<DT> reads it
template <int DT> struct SegRaw;
template <> struct SegRaw<URHGPU_DT_F32> { using T = float2; };
template <> struct SegRaw<URHGPU_DT_I8> { using T = char2; };
template <> struct SegRaw<URHGPU_DT_U8> { using T = uchar2; };
template <> struct SegRaw<URHGPU_DT_I16> { using T = short2; };
template <> struct SegRaw<URHGPU_DT_U16> { using T = ushort2; };

template <int DT>
__global__ __launch_bounds__(64) void k_batch_segments(const BatchSegArgs b) {
    using Raw = typename SegRaw<DT>::T;
    const int lane = (int)threadIdx.x;
    if ((int64_t)blockIdx.x >= b.k) return;
    const int64_t c = b.plan[2 * b.k + blockIdx.x];            // launch order: longest capture first
    if (c < 0 || c >= b.k) return;
    const BatchSegCapture cap = batch_seg_capture(b, c);
    const uint32_t n = (uint32_t)cap.n;                        // < 2^31
    const float thr = b.thr[c];                                // (a uniform address; NaN: nothing compares greater, no segment)
    const Raw *iq = (const Raw *)b.iq + cap.s0;
    int64_t *seg = b.seg + 2 * (cap.cap > 0 ? cap.roff : 0);

    // ---- segment_messages_from_magnitudes' variables, wave-uniform ----
    int state = -1;                       // 1 above the noise, -1 in it
    int64_t conseq_above = 0, conseq_below = 0, start = 0, count = 0;
    // result.append((start, end)): lane 0's pair, bounded by the region's capacity
#define BATCH_SEG_APPEND(end_) \
    do { \
        if (count < cap.cap && lane == 0) { seg[2 * count] = start; seg[2 * count + 1] = (end_); } \
        ++count; \
    } while (0)

    Raw nxt = {};
    if ((uint32_t)lane < n) nxt = iq[lane];
    for (uint32_t base = 0; base < n; base += kBatchSegStep) {
        const Raw cur = nxt;
        const uint32_t i = base + (uint32_t)lane;
        if (i + kBatchSegStep < n) nxt = iq[i + kBatchSegStep];                    // the next step's samples are on their way during this one's walk
        const bool above = i < n && seg_above<DT>(&cur, 0, thr);                   // (the sample in its register: the same comparison)
        const uint64_t m = __builtin_amdgcn_ballot_w64(above);
        const int cnt = (int)((n - base < kBatchSegStep) ? (n - base) : kBatchSegStep);
        if (base == 0) state = (m & 1ull) ? 1 : -1;                                // :77
        // a step that is one run: nothing can change where the state agrees with it
        if (state == -1 && m == 0ull) { conseq_above = 0; continue; }
        if (state == 1 && __builtin_popcountll(m) == cnt) { conseq_below = 0; continue; }
        // the step's runs of equal bits, one after the other: L samples, the first of them sample base + pos
        int pos = 0;
        while (pos < cnt) {
            const bool bit = (m >> pos) & 1ull;
            const uint64_t other = (bit ? ~m : m) >> pos;                          // the first bit of the other kind ends the run
            int L = other ? (int)__builtin_ctzll(other) : 64;
            if (L > cnt - pos) L = cnt - pos;
            const int64_t at = (int64_t)base + pos;
            if (state == 1) {
                if (bit) conseq_below = 0;                                         // :84-85
                else if (conseq_below + L >= kSegOutlierTolerance) {               // :95-100 at the run's sample that makes ten
                    const int64_t i_sw = at + (kSegOutlierTolerance - conseq_below) - 1;
                    BATCH_SEG_APPEND(i_sw - kSegOutlierTolerance);
                    state = -1;
                    conseq_below = conseq_above = 0;                               // (the rest of the run is noise in state -1: conseq_above stays 0)
                } else conseq_below += L;                                          // :86-87
            } else {
                if (!bit) conseq_above = 0;                                        // :91-92
                else if (conseq_above + L >= kSegOutlierTolerance) {               // :101-105
                    const int64_t i_sw = at + (kSegOutlierTolerance - conseq_above) - 1;
                    state = 1;
                    start = i_sw - kSegOutlierTolerance;
                    conseq_below = conseq_above = 0;                               // (the rest of the run is signal in state 1: conseq_below stays 0)
                } else conseq_above += L;                                          // :89-90
            }
            pos += L;
        }
    }
    if (n > 0 && state == 1 && start < (int64_t)n - conseq_below) BATCH_SEG_APPEND((int64_t)n - conseq_below);      // :108-109
#undef BATCH_SEG_APPEND
    if (lane == 0) b.counts[c] = count;
}

__device__ __forceinline__ int64_t batch_seg_stored(const BatchSegArgs &b, int64_t c) {
    const BatchSegCapture cap = batch_seg_capture(b, c);
    const int64_t cnt = b.counts[c];
    return cnt < 0 ? 0 : (cnt < cap.cap ? cnt : cap.cap);
}

// dir[i] = segments stored for the captures before i; dir[k] = all of them.  One workgroup: thread t owns a contiguous stretch.
__global__ __launch_bounds__(256) void k_batch_seg_scan(const BatchSegArgs b) {
    __shared__ int64_t part[256];
    const int t = (int)threadIdx.x;
    const int64_t per = (b.k + 255) / 256, lo = (t * per < b.k) ? t * per : b.k, hi = (lo + per < b.k) ? lo + per : b.k;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += batch_seg_stored(b, i);
    part[t] = sum;
    __syncthreads();
    int64_t off = 0;
    for (int j = 0; j < t; ++j) off += part[j];
    for (int64_t i = lo; i < hi; ++i) { b.dir[i] = off; off += batch_seg_stored(b, i); }
    if (t == 255) b.dir[b.k] = off;
}

// capture c's stored pairs to out[dir[c] ..): a wavefront per capture, the grid striding over the captures
__global__ __launch_bounds__(64) void k_batch_seg_pack(const BatchSegArgs b) {
    const int lane = (int)threadIdx.x;
    for (int64_t c = blockIdx.x; c < b.k; c += gridDim.x) {
        const BatchSegCapture cap = batch_seg_capture(b, c);
        const int64_t at = b.dir[c], m = b.dir[c + 1] - at;
        if (at < 0 || m <= 0 || m > cap.cap || at > b.cap_out || m > b.cap_out - at) continue;      // (the fetch reports what did not fit)
        const longlong2 *in = (const longlong2 *)(b.seg + 2 * cap.roff);
        longlong2 *o = (longlong2 *)(b.out + 2 * at);
        for (int64_t j = lane; j < m; j += 64) o[j] = in[j];
    }
}

static int launch_batch_segments(const BatchSegArgs &b, int dtype, unsigned grid, hipStream_t s) {
    return dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_batch_segments<dt.value>, dim3(grid), dim3(64), 0, s, b);
        return URHGPU_OK;
    });
}

}  // namespace urh

using namespace urh;

extern "C" {

int64_t urhgpu_batch_segments_capacity(int64_t n) { return n < 0 ? 0 : n / (2 * kSegOutlierTolerance) + 1; }

int urhgpu_batch_segments_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                              const float *d_thr, const int64_t *d_region, int64_t *d_seg, int64_t cap_seg, int64_t *d_counts, int64_t *d_dir,
                              int64_t *d_out, int64_t cap_out) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0 || cap_seg < 0 || cap_out < 0 || !d_dir) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (k > 0 && (!d_start || !d_plan || !d_thr || !d_region || !d_counts)) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || (cap_seg > 0 && !d_seg) || (cap_out > 0 && !d_out)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)d_seg & 15) || ((uintptr_t)d_out & 15) || ((uintptr_t)d_thr & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_region & 7) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_dir & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    BatchSegArgs b;
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.thr = d_thr; b.region = d_region; b.k = k; b.total = total;
    b.seg = d_seg; b.cap_seg = cap_seg; b.counts = d_counts; b.dir = d_dir; b.out = d_out; b.cap_out = cap_out;
    // three launches whatever k and the lengths are (k = 0: grids of one workgroup that finds nothing to do; the scan writes dir[0] = 0)
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    URH_TRY(launch_batch_segments(b, dtype, grid, ctx->stream));
    hipLaunchKernelGGL(k_batch_seg_scan, dim3(1), dim3(256), 0, ctx->stream, b);
    hipLaunchKernelGGL(k_batch_seg_pack, dim3(std::min<unsigned>(grid, kSegPackGrid)), dim3(64), 0, ctx->stream, b);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_segments_fetch(urhgpu_ctx *ctx, const int64_t *d_dir, int64_t k, const int64_t *d_out, int64_t *h_dir, int64_t *h_out, int64_t cap_host,
                                int64_t *n_segments) {
    if (!ctx || !d_dir || k < 0 || !h_dir || cap_host < 0 || !n_segments) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemcpyAsync(h_dir, d_dir, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    const int64_t m = h_dir[k];
    *n_segments = m;
    if (m < 0) return URHGPU_ERR_ARG;
    if (m > cap_host) return URHGPU_ERR_CAPACITY;
    if (m == 0) return URHGPU_OK;
    if (!d_out || !h_out) return URHGPU_ERR_ARG;
    URH_HIP(hipMemcpyAsync(h_out, d_out, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
