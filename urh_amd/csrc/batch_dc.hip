// batch_dc.hip -- DC correction of a batch of captures: out_c = x_c - mean(x_c, axis 0) for every capture c, bit-equal with numpy's expression
// (Filter.py:31-35, Device.py:822-823) and with urhgpu_dc_correct_dev on that capture alone, in TWO launches whatever the number of captures
// (include/urhgpu.h "a batch of captures: DC correction per capture").
//
// The correction of one capture (dc_correct.hip) evaluates numpy's strictly sequential float32 column sum by speculating on the entries of
// 4096-sample chunks and stitching them: up to five launches and a work area per context, which only pays on captures far longer than a
// batch's.  In a batch the parallelism is ACROSS captures, as for the Costas loop (batch_psk.hip):
//
//   k_batch_dc_mean<float>   the recurrence s = fl32(s + x[i]) from +0.0 in index order, nothing speculated, nothing reassociated: a LANE per
//       (capture, column), a wavefront (= a workgroup) per 32 captures taken in the plan's launch order (longest first: the lanes of a
//       wavefront hold captures of similar length).  A lane reading its own capture from global memory would touch 64 cache lines per
//       instruction, so the samples are staged through LDS in tiles of 128: for r = 0 .. 31 the wavefront loads 128 consecutive samples of
//       capture r with two coalesced loads and stores their I and Q components as rows 2 r and 2 r + 1 of the tile; then lane l walks row l.
//       The row stride is 129 words (odd), so the 32 lanes of a half-wavefront read distinct banks in every step.  The loads of the NEXT
//       tile are issued into registers before the walk, and the walk reads its row into registers ahead of the additions: only the adds are
//       on the dependent chain.  The rows' pointers and lengths live in registers, not in LDS tables read in front of every load.  Samples past a capture's end are filled in as -0.0, the identity of the addition (s + -0.0 == s for every
//       s, -0.0 and NaN included): a lane past its end keeps its sum without a select on the chain.  mean = (float)((double)s / (double)n),
//       as at the end of k_dc_stitch.
//   k_batch_dc_mean<T>       (integers) a workgroup per capture in the same order: exact int64 column sums (16-byte vectors between the
//       capture's first and last 16-byte boundary, at most eight terms in an int32 before they reach the int64), a block reduction,
//       mean = double(sum) / double(n).
//   k_batch_dc_sub<T, M>     out = x - mean, one streaming launch over all captures: workgroup (x, y) takes every gridDim.y-th stretch of
//       capture x, 16-byte vectors where the capture allows (its start is aligned to a sample only), dc_sub per component.  In place or
//       into a buffer of the same geometry; what lies between the captures is neither read nor written.
// No atomics, no workgroup waits for another, nothing waits for the host.  An empty capture stores nothing but its mean, 0 / 0 = NaN.
#include "batch_kernels.hpp"      // (first: the fp64 forms of URH_FDIV / URH_FSQRT)

#include <algorithm>

#include "dc_sub.hpp"

namespace urh {

constexpr int kBdCaps = 32;                // captures per wavefront of the float32 mean: a lane per (capture, column)
constexpr int kBdTile = 128;               // samples per tile: two coalesced loads per row
constexpr int kBdStride = kBdTile + 1;     // row stride in words: odd, the lanes of a step read distinct banks
constexpr int kBdBlock = 256;              // threads of the integer mean and of the subtraction
constexpr int kBdParts = 8;                // workgroups that share a capture's subtraction

// the capture of launch slot `slot`, or nullptr-like (c = -1): what k_batch_costas reads of the plan
__device__ __forceinline__ int64_t bd_capture_of(const BatchArgs &b, int64_t slot) {
    if (slot >= b.k) return -1;
    const int64_t c = b.plan[2 * b.k + slot];              // launch order: longest capture first
    return (c >= 0 && c < b.k) ? c : -1;
}

template <class T>
__global__ __launch_bounds__(kBdBlock) void k_batch_dc_mean(const BatchArgs b, void *mean_out) {
    constexpr int kPer = 16 / (int)sizeof(T);              // components in a vector: I, Q, I, Q, ...
    __shared__ long long s_w[2][kBdBlock / 64];
    const int tid = (int)threadIdx.x;
    const int64_t c = bd_capture_of(b, blockIdx.x);
    if (c < 0) return;
    const BatchCapture cap = batch_capture(b, c);          // (a start or an end that is refused: n = 0, nothing is read)
    const int64_t n = cap.n;
    const T *in = (const T *)b.iq + 2 * cap.s0;
    const int sample = 2 * (int)sizeof(T);
    const int64_t head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)in & 15)) & 15) / sample));
    const int64_t nvec = (n - head) * sample / 16;
    long long sum_i = 0, sum_q = 0;
    const uint4 *v = (const uint4 *)(in + 2 * head);
    for (int64_t i = tid; i < nvec; i += kBdBlock) {
        const uint4 w = v[i];
        T e[kPer];
        __builtin_memcpy(e, &w, 16);
        int a_i = 0, a_q = 0;                              // at most eight terms of 16 bits
#pragma unroll
        for (int j = 0; j < kPer; j += 2) { a_i += (int)e[j]; a_q += (int)e[j + 1]; }
        sum_i += a_i;
        sum_q += a_q;
    }
    const int64_t body_end = head + nvec * (kPer / 2), n_scalar = head + (n - body_end);
    for (int64_t i = tid; i < n_scalar; i += kBdBlock) {
        const int64_t j = i < head ? i : body_end + (i - head);
        sum_i += (int)in[2 * j];
        sum_q += (int)in[2 * j + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum_i += __shfl_down(sum_i, o, 64); sum_q += __shfl_down(sum_q, o, 64); }
    if ((tid & 63) == 0) { s_w[0][tid >> 6] = sum_i; s_w[1][tid >> 6] = sum_q; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kBdBlock / 64; ++w) { sum_i += s_w[0][w]; sum_q += s_w[1][w]; }
    double *mean = (double *)mean_out + 2 * c;
    mean[0] = (double)sum_i / (double)n;                   // (n = 0: NaN, as numpy gives)
    mean[1] = (double)sum_q / (double)n;
}

template <>
__global__ __launch_bounds__(64) void k_batch_dc_mean<float>(const BatchArgs b, void *mean_out) {
    __shared__ float tile[2 * kBdCaps * kBdStride];        // row 2 r + column of capture r: 33 024 bytes
    __shared__ int64_t s_s0[kBdCaps];                      // row pair r: its capture's first sample ...
    __shared__ uint32_t s_n[kBdCaps];                      // ... and its samples (0: none)
    const int lane = (int)threadIdx.x, r_mine = lane >> 1, col = lane & 1;
    const int64_t c = bd_capture_of(b, (int64_t)blockIdx.x * kBdCaps + r_mine);
    int64_t s0 = 0;
    uint32_t n_mine = 0;                                   // < 2^31
    if (c >= 0) {
        const BatchCapture cap = batch_capture(b, c);      // (n is the samples' alone: a refused start or end is an empty capture)
        s0 = cap.s0;
        n_mine = (uint32_t)cap.n;
    }
    if (col == 0) { s_s0[r_mine] = s0; s_n[r_mine] = n_mine; }
    uint32_t n_end = n_mine;                               // the wavefront's longest capture
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_end = max(n_end, (uint32_t)__shfl_xor((int)n_end, o));
    n_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_end);
    __syncthreads();

    const float2 none = make_float2(-0.0f, -0.0f);         // the addition's identity: what a row holds past its capture's end
    // row pair r in registers, read from the tables once: this lane's sample of its capture's current tile, and the capture's length.  (Read
    // from LDS in front of every load, each row's table entries cost the fill an LDS round trip of their own.)
    const float2 *p[kBdCaps];
    uint32_t nr[kBdCaps];
#pragma unroll
    for (int r = 0; r < kBdCaps; ++r) { p[r] = (const float2 *)b.iq + s_s0[r] + lane; nr[r] = s_n[r]; }
    float2 v[2 * kBdCaps];
    // row pair r of the tile at `base`: 128 consecutive samples of capture r, two coalesced loads (sample indices are unsigned 32-bit: a
    // capture holds up to 2^31 - 1 samples, and base + 128 does not wrap for the longest of them); then on to the next tile
#define BD_LOAD(base_)                                                                            \
    {                                                                                             \
        const uint32_t i0 = (base_) + (uint32_t)lane, i1 = i0 + 64u;                              \
        _Pragma("unroll") for (int r = 0; r < kBdCaps; ++r) {                                     \
            v[2 * r] = none;                                                                      \
            v[2 * r + 1] = none;                                                                  \
            if (i0 < nr[r]) v[2 * r] = p[r][0];                                                   \
            if (i1 < nr[r]) v[2 * r + 1] = p[r][64];                                              \
            p[r] += kBdTile;                                                                      \
        }                                                                                         \
    }
    BD_LOAD(0u)
    float s = 0.0f;                                        // +0.0: numpy's accumulator starts there
    for (uint32_t base = 0; base < n_end; base += kBdTile) {
#pragma unroll
        for (int r = 0; r < kBdCaps; ++r) {
            tile[(2 * r) * kBdStride + lane] = v[2 * r].x;
            tile[(2 * r) * kBdStride + 64 + lane] = v[2 * r + 1].x;
            tile[(2 * r + 1) * kBdStride + lane] = v[2 * r].y;
            tile[(2 * r + 1) * kBdStride + 64 + lane] = v[2 * r + 1].y;
        }
        __syncthreads();
        if (base + kBdTile < n_end) BD_LOAD(base + kBdTile)          // the next tile's loads fly during the walk
        // ---- 128 steps: lane l follows row l; the row is read ahead of the additions ----
#pragma unroll
        for (int u0 = 0; u0 < kBdTile; u0 += 64) {
            float x[64];
#pragma unroll
            for (int u = 0; u < 64; ++u) x[u] = tile[lane * kBdStride + u0 + u];
#pragma unroll
            for (int u = 0; u < 64; ++u) s += x[u];
        }
        __syncthreads();                                   // (the next iteration rewrites the tile)
    }
#undef BD_LOAD
    if (c >= 0) ((float *)mean_out)[2 * c + col] = (float)((double)s / (double)n_mine);     // numpy: the float32 sum divided in float64, rounded once
}

template <class T, class M>
__global__ __launch_bounds__(kBdBlock) void k_batch_dc_sub(const BatchArgs b, T *out_all, const M *mean) {
    constexpr int kPer = 16 / (int)sizeof(T);
    const int64_t c = bd_capture_of(b, blockIdx.x);
    if (c < 0) return;
    const BatchCapture cap = batch_capture(b, c);
    const int64_t n = cap.n;
    if (n == 0) return;
    const M m_i = mean[2 * c], m_q = mean[2 * c + 1];
    const T *in = (const T *)b.iq + 2 * cap.s0;
    T *out = out_all + 2 * cap.s0;                         // (the two buffers are aligned alike: 16 bytes at sample 0)
    const int sample = 2 * (int)sizeof(T);
    const int64_t head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)in & 15)) & 15) / sample));
    const int64_t nvec = (n - head) * sample / 16;
    const int64_t gid = (int64_t)blockIdx.y * kBdBlock + threadIdx.x, stride = (int64_t)gridDim.y * kBdBlock;
    const uint4 *v = (const uint4 *)(in + 2 * head);
    uint4 *o = (uint4 *)(out + 2 * head);
    for (int64_t i = gid; i < nvec; i += stride) {
        uint4 w = v[i];
        T e[kPer];
        __builtin_memcpy(e, &w, 16);
#pragma unroll
        for (int j = 0; j < kPer; j += 2) { e[j] = dc_sub(e[j], m_i); e[j + 1] = dc_sub(e[j + 1], m_q); }
        __builtin_memcpy(&w, e, 16);
        o[i] = w;
    }
    const int64_t body_end = head + nvec * (kPer / 2), n_scalar = head + (n - body_end);
    for (int64_t i = gid; i < n_scalar; i += stride) {
        const int64_t j = i < head ? i : body_end + (i - head);
        const T x_i = in[2 * j], x_q = in[2 * j + 1];
        out[2 * j] = dc_sub(x_i, m_i);
        out[2 * j + 1] = dc_sub(x_q, m_q);
    }
}

template <class T>
static void launch_batch_dc(const BatchArgs &b, void *d_out, void *d_mean, hipStream_t s) {
    const unsigned k = (unsigned)b.k;
    if constexpr (std::is_same<T, float>::value) {
        hipLaunchKernelGGL(k_batch_dc_mean<float>, dim3((k + kBdCaps - 1) / kBdCaps), dim3(64), 0, s, b, d_mean);
        hipLaunchKernelGGL((k_batch_dc_sub<float, float>), dim3(k, kBdParts), dim3(kBdBlock), 0, s, b, (float *)d_out, (const float *)d_mean);
    } else {
        hipLaunchKernelGGL(k_batch_dc_mean<T>, dim3(k), dim3(kBdBlock), 0, s, b, d_mean);
        hipLaunchKernelGGL((k_batch_dc_sub<T, double>), dim3(k, kBdParts), dim3(kBdBlock), 0, s, b, (T *)d_out, (const double *)d_mean);
    }
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_dc_correct_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan,
                                int64_t k, void *d_out, void *d_mean) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0 || total > (int64_t(1) << 40)) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (k > 0 && (!d_start || !d_plan)) return URHGPU_ERR_ARG;
    if ((total > 0 && (!d_iq || !d_out)) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_out & 15)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_mean & 7)) return URHGPU_ERR_ARG;
    const int comp = dtype == URHGPU_DT_F32 ? 4 : (dtype == URHGPU_DT_I16 || dtype == URHGPU_DT_U16) ? 2 : 1;
    const size_t bytes = (size_t)total * 2 * comp;
    if (d_iq != d_out && (const char *)d_iq < (const char *)d_out + bytes && (const char *)d_out < (const char *)d_iq + bytes) return URHGPU_ERR_ARG;
    if (k == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    if (!d_mean) {                                         // the means live in the context between the two launches
        URH_TRY(ctx->batch_dc_mean.reserve((size_t)k * 16));
        d_mean = ctx->batch_dc_mean.base;
    }
    BatchArgs b;
    memset(&b, 0, sizeof(b));                              // no work buffer: batch_capture then vouches for the samples alone
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total;
    b.sps = 1; b.bps = 1;
    URH_TRY(dispatch_dtype(dtype, [&](auto dt) {           // (the range check above has refused every other code)
        launch_batch_dc<typename decltype(dt)::type>(b, d_out, d_mean, ctx->stream);
        return URHGPU_OK;
    }));
    ctx->batch_launches += 2;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // extern "C"
