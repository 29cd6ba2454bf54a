// chunk_stats.hip -- one pass over a chunk of the live sniffer (ProtocolSniffer.__demodulate_data,
// src/urh/signalprocessing/ProtocolSniffer.py:204-281) for gfx950.
//
// The reference receives `data`, the raw real (n, 2) array of the device's dtype, and gates it on
//     power_spectrum = data.real ** 2.0 + data.imag ** 2.0        (== data ** 2.0: .imag of a real array is zeros)
//     np.sqrt(np.mean(power_spectrum)) > noise_threshold,   0.1 * np.sqrt(np.max(power_spectrum)) for the adaptive threshold
// before it appends the chunk to its accumulation buffer.  One read of the chunk here does both:
//   (a) the chunk's rows -- the first n_store of them when the buffer is nearly full (the reference trims the append) -- are stored to the
//       accumulation buffer (d_dst; skipped when the chunk already lies there), and
//   (b) the sum and the maximum of the 2n squares are formed in the reference's arithmetic:
//       float32   float32 squares, summed in numpy's pairwise order (pairwise.hpp), maximum as np.max (NaN propagates);
//       integers  float64 squares in numpy; all of them are exact integers, so a 64-bit integer sum equals numpy's float64 sum
//                 whenever the total stays below 2^53 (every partial sum is then exact, whatever the order).
// Two launches whatever the chunk's length: per-workgroup partials, then one workgroup that combines them and stores the two
// results (as float64) into pinned host memory with ordinary stores.  No float atomics: the order of the float32 sum is fixed.
//
// A live chunk is a slice of a larger buffer: the source starts on a row boundary (2 bytes for int8), the destination on another,
// so the 16-byte accesses are issued without an alignment promise (the hardware takes unaligned dwordx4 addresses).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"
#include "pairwise.hpp"

namespace urh {

struct alignas(1) Bytes16 { unsigned char b[16]; };
template <typename V>
__device__ __forceinline__ V load16(const void *p) { V v; __builtin_memcpy(&v, p, 16); return v; }
template <typename V>
__device__ __forceinline__ void store16(void *p, const V &v) { __builtin_memcpy(p, &v, 16); }

// np.max over floats: the first NaN wins.  Kept as (maximum of the non-NaN values, NaN seen).
__device__ __forceinline__ void fmax_nan(float &mx, bool &nan, float v) {
    nan = nan || (v != v);
    if (v > mx) mx = v;
}

// ---- float32 -----------------------------------------------------------------------------------------------------------------
// One workgroup per piece of kPwChunk floats (numpy's reduction buffer): the piece is read with coalesced 16-byte loads, stored to
// the destination, squared into LDS, and the piece's pairwise tree is evaluated from there.  LDS index of element e: e + 8 * (e /
// 128), so that the four threads per leaf of 16 neighbouring leaves do not meet on one bank (leaf stride 136 dwords) while
// 16-byte stores stay aligned.
constexpr int kCsBlock = 256;
constexpr int kCsLdsFloats = kPwChunk + 8 * kPwLeavesPerChunk;
constexpr int kCsLevels = 7;                                   // depth of pw's tree over fewer than kPwChunk elements (see the irregular piece below)
__device__ __forceinline__ int cs_lds(int e) { return e + ((e >> 7) << 3); }

__global__ __launch_bounds__(kCsBlock) void k_chunk_stats_f32(const float *src, int64_t nf, float *dst, int64_t n_store, float *part_sum, float *part_max) {
    __shared__ __attribute__((aligned(16))) float s_sq[kCsLdsFloats];
    __shared__ float s_leaf[kPwLeavesPerChunk];
    __shared__ int s_off[2][1 << kCsLevels], s_len[2][1 << kCsLevels];
    __shared__ unsigned char s_split[kCsLevels][1 << kCsLevels];
    __shared__ float s_val[2][1 << kCsLevels], s_wmax[kCsBlock / 64];
    __shared__ int s_wnan[kCsBlock / 64];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kPwChunk;
    const int len = (nf - base < kPwChunk) ? (int)(nf - base) : kPwChunk;
    const float *x = src + base;
    float *y = dst + base;
    const int64_t lim = n_store - base;                        // elements of this piece that are stored (<= 0: none; dst == nullptr: n_store == 0)
    float mx = -INFINITY;
    bool nan = false;
#pragma unroll
    for (int it = 0; it < kPwChunk / (4 * kCsBlock); ++it) {
        const int e = 4 * (it * kCsBlock + t);
        if (e + 4 <= len) {
            const float4 v = load16<float4>(x + e);
            if (e + 4 <= lim) store16(y + e, v);
            else if (e + 2 <= lim) { y[e] = v.x; y[e + 1] = v.y; }        // the stored part ends on a row (two floats)
            float4 q;
            q.x = v.x * v.x; q.y = v.y * v.y; q.z = v.z * v.z; q.w = v.w * v.w;
            fmax_nan(mx, nan, q.x); fmax_nan(mx, nan, q.y); fmax_nan(mx, nan, q.z); fmax_nan(mx, nan, q.w);
            *(float4 *)&s_sq[cs_lds(e)] = q;
        } else {
            for (int k = e; k < len; ++k) {                   // the piece's last (partial) 16 bytes
                const float v = x[k];
                if (k < lim) y[k] = v;
                const float q = v * v;
                fmax_nan(mx, nan, q);
                s_sq[cs_lds(k)] = q;
            }
        }
    }
    // maximum: wavefront reduction, then across the four wavefronts
    int nan_i = nan ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mx, o);
        nan_i |= __shfl_xor(nan_i, o);
        if (a > mx) mx = a;
    }
    if ((t & 63) == 0) { s_wmax[t >> 6] = mx; s_wnan[t >> 6] = nan_i; }
    __syncthreads();

    float total = 0.f;
    if (len == kPwChunk) {
        // a full piece: leaf L = t / 4, accumulators 2q and 2q + 1 with q = t % 4
        const int L = t >> 2, q = t & 3;
        const float *a = &s_sq[L * (kPwLeaf + 8) + 2 * q];
        float r0 = a[0], r1 = a[1];
#pragma unroll
        for (int i = 8; i < kPwLeaf; i += 8) { r0 += a[i]; r1 += a[i + 1]; }
        float p = r0 + r1;                                       // (r[2q] + r[2q+1])
        p = p + __shfl_xor(p, 1);                                // (r0 + r1) + (r2 + r3)   |   (r4 + r5) + (r6 + r7)
        p = p + __shfl_xor(p, 2);                                // the leaf (float addition commutes: both halves hold the same value)
        if (q == 0) s_leaf[L] = p;
        __syncthreads();
        if (t < 64) {
            float s = s_leaf[t];                                 // perfect binary tree over the 64 leaves, neighbours first
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
            total = s;
        }
    } else {
        // the irregular last piece: pw's tree, level by level.  Level d holds up to 2^d nodes (offset, length); a node longer than a leaf
        // splits by pw's own rule into the slots 2i and 2i + 1 of the next level, a leaf moves on to slot 2i alone.  Lengths shrink to
        // at most n / 2 + 7.5 per level, so after kCsLevels levels every node is a leaf; they are summed one per thread (pw_leaf) and
        // the sums travel back up, added wherever a node had split -- left + right, as pw adds them.
        if (t == 0) { s_off[0][0] = 0; s_len[0][0] = len; }
        for (int d = 0; d < kCsLevels; ++d) {
            __syncthreads();
            if (t < (1 << d)) {
                const int o = s_off[d & 1][t], n = s_len[d & 1][t];
                const bool split = n > kPwLeaf;
                const int n2 = split ? (int)pw_split(n) : n;
                s_off[(d + 1) & 1][2 * t] = o; s_len[(d + 1) & 1][2 * t] = n2;
                s_off[(d + 1) & 1][2 * t + 1] = o + n2; s_len[(d + 1) & 1][2 * t + 1] = n - n2;      // length 0: no node
                s_split[d][t] = split ? 1 : 0;
            }
        }
        __syncthreads();
        if (t < (1 << kCsLevels)) {
            const int o = s_off[kCsLevels & 1][t], n = s_len[kCsLevels & 1][t];
            s_val[kCsLevels & 1][t] = n > 0 ? pw_leaf(n, [&](int i) { return s_sq[cs_lds(o + i)]; }) : 0.f;
        }
        for (int d = kCsLevels - 1; d >= 0; --d) {
            __syncthreads();
            if (t < (1 << d)) {
                const float l = s_val[(d + 1) & 1][2 * t], r = s_val[(d + 1) & 1][2 * t + 1];
                s_val[d & 1][t] = s_split[d][t] ? l + r : l;
            }
        }
        if (t == 0) total = s_val[0][0];
    }
    if (t == 0) {
        for (int w = 1; w < kCsBlock / 64; ++w) { if (s_wmax[w] > mx) mx = s_wmax[w]; nan_i |= s_wnan[w]; }
        part_sum[blockIdx.x] = total;
        part_max[blockIdx.x] = nan_i ? NAN : mx;
    }
}

// total = (((0 + piece 0) + piece 1) + ...) in float32, by one thread out of LDS; the maximum over all workgroups
__global__ __launch_bounds__(kCsBlock) void k_chunk_finish_f32(const float *part_sum, const float *part_max, int nb, double *h_out) {
    __shared__ float s_part[4096];
    __shared__ float s_wmax[kCsBlock / 64];
    __shared__ int s_wnan[kCsBlock / 64];
    const int t = threadIdx.x;
    float mx = -INFINITY;
    bool nan = false;
    for (int b = t; b < nb; b += kCsBlock) fmax_nan(mx, nan, part_max[b]);
    int nan_i = nan ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_xor(mx, o);
        nan_i |= __shfl_xor(nan_i, o);
        if (a > mx) mx = a;
    }
    if ((t & 63) == 0) { s_wmax[t >> 6] = mx; s_wnan[t >> 6] = nan_i; }
    float total = 0.f;
    for (int b0 = 0; b0 < nb; b0 += 4096) {
        const int m = min(nb - b0, 4096);
        __syncthreads();
        for (int b = t; b < m; b += kCsBlock) s_part[b] = part_sum[b0 + b];
        __syncthreads();
        if (t == 0) for (int b = 0; b < m; ++b) total = total + s_part[b];
    }
    if (t == 0) {
        for (int w = 1; w < kCsBlock / 64; ++w) { if (s_wmax[w] > mx) mx = s_wmax[w]; nan_i |= s_wnan[w]; }
        h_out[0] = (double)total;
        h_out[1] = nan_i ? (double)NAN : (double)mx;
        h_out[2] = 0.0;
    }
}

// ---- integer sample types ----------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ uint32_t sq_u32(T v) {
    const int32_t w = (int32_t)v;                   // |v| <= 65535: the square fits 32 unsigned bits
    return (uint32_t)w * (uint32_t)w;
}
constexpr int kCsIntLoads = 4;                       // 16-byte loads per thread: 16 KiB per workgroup

template <typename T>
__global__ __launch_bounds__(kCsBlock) void k_chunk_stats_int(const T *src, int64_t ne, T *dst, int64_t n_store, unsigned long long *part_sum, uint32_t *part_max) {
    constexpr int kPer = 16 / (int)sizeof(T);
    __shared__ unsigned long long s_wsum[kCsBlock / 64];
    __shared__ uint32_t s_wmax[kCsBlock / 64];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (kCsBlock * kCsIntLoads * kPer);
    unsigned long long sum = 0;
    uint32_t mx = 0;
#pragma unroll
    for (int it = 0; it < kCsIntLoads; ++it) {
        const int64_t e = base + (int64_t)(it * kCsBlock + t) * kPer;
        if (e + kPer <= ne) {
            const Bytes16 raw = load16<Bytes16>(src + e);
            if (e + kPer <= n_store) store16(dst + e, raw);
            else for (int64_t k = e; k < n_store; ++k) dst[k] = src[k];       // the stored part ends inside these 16 bytes
            T v[kPer];
            __builtin_memcpy(v, &raw, 16);
            uint32_t part = 0;                       // 8-bit samples: 16 squares <= 2^14 fit 32 bits; 16-bit squares go to the 64-bit sum one by one
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const uint32_t q = sq_u32(v[k]);
                if (q > mx) mx = q;
                if (sizeof(T) == 1) part += q; else sum += q;
            }
            sum += part;
        } else {
            for (int64_t k = e; k < ne; ++k) {       // the chunk's last (partial) 16 bytes
                const T v = src[k];
                if (k < n_store) dst[k] = v;
                const uint32_t q = sq_u32(v);
                if (q > mx) mx = q;
                sum += q;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        const uint32_t a = (uint32_t)__shfl_xor((int)mx, o);
        if (a > mx) mx = a;
    }
    if ((t & 63) == 0) { s_wsum[t >> 6] = sum; s_wmax[t >> 6] = mx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kCsBlock / 64; ++w) { sum += s_wsum[w]; if (s_wmax[w] > mx) mx = s_wmax[w]; }
        part_sum[blockIdx.x] = sum;
        part_max[blockIdx.x] = mx;
    }
}

// h_out[2] carries the exact integer total (as two 32-bit halves would not survive a double): the host refuses totals >= 2^53
__global__ __launch_bounds__(kCsBlock) void k_chunk_finish_int(const unsigned long long *part_sum, const uint32_t *part_max, int nb, double *h_out) {
    __shared__ unsigned long long s_wsum[kCsBlock / 64];
    __shared__ uint32_t s_wmax[kCsBlock / 64];
    const int t = threadIdx.x;
    unsigned long long sum = 0;
    uint32_t mx = 0;
    for (int b = t; b < nb; b += kCsBlock) { sum += part_sum[b]; if (part_max[b] > mx) mx = part_max[b]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        const uint32_t a = (uint32_t)__shfl_xor((int)mx, o);
        if (a > mx) mx = a;
    }
    if ((t & 63) == 0) { s_wsum[t >> 6] = sum; s_wmax[t >> 6] = mx; }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kCsBlock / 64; ++w) { sum += s_wsum[w]; if (s_wmax[w] > mx) mx = s_wmax[w]; }
        h_out[0] = (double)sum;
        h_out[1] = (double)mx;
        h_out[2] = (sum >> 53) ? 1.0 : 0.0;          // the float64 sum of the reference is no longer the exact total
    }
}

template <typename T>
static void chunk_stats_int_launch(const void *src, int64_t ne, void *dst, int64_t n_store, void *part, int nb, double *h_out, hipStream_t s) {
    unsigned long long *ps = (unsigned long long *)part;
    uint32_t *pm = (uint32_t *)(ps + nb);
    hipLaunchKernelGGL(k_chunk_stats_int<T>, dim3((unsigned)nb), dim3(kCsBlock), 0, s, (const T *)src, ne, (T *)dst, n_store, ps, pm);
    hipLaunchKernelGGL(k_chunk_finish_int, dim3(1), dim3(kCsBlock), 0, s, ps, pm, nb, h_out);
}

static int64_t chunk_stats_blocks(int dtype, int64_t n_rows) {
    const int64_t ne = 2 * n_rows;
    if (dtype == URHGPU_DT_F32) return (ne + kPwChunk - 1) / kPwChunk;
    const int64_t per = (int64_t)kCsBlock * kCsIntLoads * (16 / ((dtype == URHGPU_DT_I8 || dtype == URHGPU_DT_U8) ? 1 : 2));
    return (ne + per - 1) / per;
}
size_t chunk_stats_scratch_bytes(int dtype, int64_t n_rows) { return (size_t)chunk_stats_blocks(dtype, n_rows) * 12 + 64; }

// d_src: n_rows rows of two samples; d_dst: nullptr (no store) or the destination of the first store_rows rows (no overlap with the
// source); h_out: three doubles in pinned host memory {sum, max, sum not exact}, valid once the stream has drained.  Two launches.
int launch_chunk_stats(const void *d_src, int dtype, int64_t n_rows, void *d_dst, int64_t store_rows, void *scratch, double *h_out, hipStream_t s) {
    if (n_rows <= 0 || n_rows > (int64_t(1) << 31) || store_rows < 0 || store_rows > n_rows) return URHGPU_ERR_ARG;
    const int64_t ne = 2 * n_rows, ns = d_dst ? 2 * store_rows : 0;
    const int nb = (int)chunk_stats_blocks(dtype, n_rows);
    return dispatch_dtype(dtype, [&](auto dt) {
        if constexpr (dt.value == URHGPU_DT_F32) {
            float *ps = (float *)scratch, *pm = ps + nb;
            hipLaunchKernelGGL(k_chunk_stats_f32, dim3((unsigned)nb), dim3(kCsBlock), 0, s, (const float *)d_src, ne, (float *)d_dst, ns, ps, pm);
            hipLaunchKernelGGL(k_chunk_finish_f32, dim3(1), dim3(kCsBlock), 0, s, ps, pm, nb, h_out);
        } else
            chunk_stats_int_launch<typename decltype(dt)::type>(d_src, ne, d_dst, ns, scratch, nb, h_out, s);
        return URHGPU_OK;
    });
}

}  // namespace urh
