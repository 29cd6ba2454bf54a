// dc_correct.hip -- DC correction: out = x - mean(x, axis 0), bit-equal with numpy's expression (Filter.py:31-35, Device.py:822-823).
//
// Integer captures: exact int64 column sums per workgroup, finished by the last workgroup (no float atomics); mean = double(sum) / double(n);
// out = (T)(int32) trunc(double(x) - mean).
//
// float32 captures: numpy reduces a C-contiguous (N, 2) array along its slow axis, so a column's sum is the strictly sequential float32
// recurrence s = fl32(s + x[i]) from +0.0.  That recurrence is evaluated in chunks of kDcChunk samples:
//   1. k_dc_chunk_sums / k_dc_prefix: float64 chunk sums and their exclusive prefix; fl32(prefix) is the GUESSED entry of a chunk.
//   2. k_dc_spec: one lane per (chunk, column) evaluates its chunk serially from the guess and from the guess's neighbour, and records of
//      both paths entry, exit, the smallest and the largest |s| on the way and whether the sign changed.
//   3. k_dc_stitch: one wavefront walks the chunks in order.  While a running sum stays inside one binade, s = k * u with an integer k, and
//      fl32(s + x) = (k + rne(x / u)) * u: the rounding does not depend on k, except for a tie's choice of the even neighbour.  So a chunk
//      entered d ulps away from its guess leaves d ulps away from the speculated exit, provided both paths stay inside the binade (|d| + 1
//      within the recorded distance from the binade's edges) and d is even -- which it is for one of the two paths.  Every other chunk is re-evaluated serially
//      from its true entry, out of LDS.  Nothing waits for the host; a capture whose chunks all fail the test costs the serial recurrence.
// Captures of at most kDcDirectMax samples skip 1. and 2.: the wavefront of 3. evaluates them directly.
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace urh {

std::atomic<long long> g_dc_host_syncs{0};

constexpr int kDcChunk = 4096;                       // samples per speculated chunk
constexpr int64_t kDcDirectMax = 2 * kDcChunk;       // at most this many samples: evaluated directly
constexpr int kDcBlock = 256;
constexpr int kDcMaxGrid = 2048;                     // workgroups of the streaming kernels (grid-stride)
constexpr int kDcSpecBatch = 32;                     // samples a speculating lane keeps in registers ahead of its additions
// the work area: header, the integer partials, then (float32) per chunk and column a double sum, a float guess and two 16-byte records
constexpr size_t kDcOffMean = 0;                     // double[2] (integers) / float[2] (float32)
constexpr size_t kDcOffTicket = 64;
constexpr size_t kDcOffStats = 128;                  // int64[4]
constexpr size_t kDcOffPart = 256;                   // long long[2 * kDcMaxGrid]
constexpr size_t kDcHeader = kDcOffPart + size_t(kDcMaxGrid) * 16;

__device__ __forceinline__ long long dc_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double dc_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// sum over the workgroup (kDcBlock threads), valid in thread 0
template <class V> __device__ __forceinline__ V dc_block_sum(V v, V *s_w) {
    v = dc_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) for (int w = 1; w < kDcBlock / 64; ++w) v += s_w[w];
    return v;
}

// The streaming kernels' view of a capture: `head` samples in front of the first 16-byte boundary, nvec 16-byte vectors, the rest behind.
struct DcSpan {
    int64_t n, head, nvec;
};

// ---- integers: column sums, mean -----------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kDcBlock) k_dc_isum(const T *__restrict__ in, DcSpan sp, long long *part, unsigned int *ticket, double *mean,
                                                       double *user_mean) {
    constexpr int kPer = 16 / (int)sizeof(T);        // components in a vector: I, Q, I, Q, ...
    __shared__ long long s_w[kDcBlock / 64];
    __shared__ bool s_last;
    long long sum_i = 0, sum_q = 0;
    const int64_t gid = (int64_t)blockIdx.x * kDcBlock + threadIdx.x, stride = (int64_t)gridDim.x * kDcBlock;
    const uint4 *v = (const uint4 *)(in + 2 * sp.head);
    for (int64_t i = gid; i < sp.nvec; i += stride) {
        const uint4 w = v[i];
        T e[kPer];
        __builtin_memcpy(e, &w, 16);
        int a_i = 0, a_q = 0;
#pragma unroll
        for (int k = 0; k < kPer; k += 2) { a_i += (int)e[k]; a_q += (int)e[k + 1]; }
        sum_i += a_i;
        sum_q += a_q;
    }
    const int64_t body_end = sp.head + sp.nvec * (kPer / 2), n_scalar = sp.head + (sp.n - body_end);
    for (int64_t i = gid; i < n_scalar; i += stride) {
        const int64_t j = i < sp.head ? i : body_end + (i - sp.head);
        sum_i += (int)in[2 * j];
        sum_q += (int)in[2 * j + 1];
    }
    sum_i = dc_block_sum(sum_i, s_w);
    sum_q = dc_block_sum(sum_q, s_w);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sum_i;
        part[2 * blockIdx.x + 1] = sum_q;
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    sum_i = 0; sum_q = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += kDcBlock) {
        sum_i += __hip_atomic_load(part + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sum_q += __hip_atomic_load(part + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sum_i = dc_block_sum(sum_i, s_w);
    sum_q = dc_block_sum(sum_q, s_w);
    if (threadIdx.x == 0) {
        const double m_i = (double)sum_i / (double)sp.n, m_q = (double)sum_q / (double)sp.n;
        mean[0] = m_i; mean[1] = m_q;
        if (user_mean) { user_mean[0] = m_i; user_mean[1] = m_q; }
        *ticket = 0;                                 // the next call's election
    }
}

// ---- the subtraction, every sample type ----------------------------------------------------------------------------------------------
template <class T, class M> __device__ __forceinline__ T dc_sub(T x, M m) {
    if constexpr (std::is_same<T, float>::value) return x - m;
    else return (T)(int)((double)x - m);             // truncated toward zero into an int32, low bits kept: numpy's cast on x86-64
}
template <class T, class M>
__global__ void __launch_bounds__(kDcBlock) k_dc_sub(const T *in, T *out, DcSpan sp, const M *mean) {
    constexpr int kPer = 16 / (int)sizeof(T);
    const M m_i = mean[0], m_q = mean[1];
    const int64_t gid = (int64_t)blockIdx.x * kDcBlock + threadIdx.x, stride = (int64_t)gridDim.x * kDcBlock;
    const uint4 *v = (const uint4 *)(in + 2 * sp.head);
    uint4 *o = (uint4 *)(out + 2 * sp.head);
    for (int64_t i = gid; i < sp.nvec; i += stride) {
        uint4 w = v[i];
        T e[kPer];
        __builtin_memcpy(e, &w, 16);
#pragma unroll
        for (int k = 0; k < kPer; k += 2) { e[k] = dc_sub(e[k], m_i); e[k + 1] = dc_sub(e[k + 1], m_q); }
        __builtin_memcpy(&w, e, 16);
        o[i] = w;
    }
    const int64_t body_end = sp.head + sp.nvec * (kPer / 2), n_scalar = sp.head + (sp.n - body_end);
    for (int64_t i = gid; i < n_scalar; i += stride) {
        const int64_t j = i < sp.head ? i : body_end + (i - sp.head);
        const T a = in[2 * j], b = in[2 * j + 1];
        out[2 * j] = dc_sub(a, m_i);
        out[2 * j + 1] = dc_sub(b, m_q);
    }
}

// ---- float32, pass 1: float64 chunk sums and their prefix ----------------------------------------------------------------------------
// sums[col * n_chunks + c]; one workgroup per chunk (grid-stride)
__global__ void __launch_bounds__(kDcBlock) k_dc_chunk_sums(const float2 *__restrict__ in, int64_t n, int64_t n_chunks, double *sums) {
    __shared__ double s_w[kDcBlock / 64];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t start = c * kDcChunk;
        const int len = (int)std::min<int64_t>(kDcChunk, n - start);
        double a_i = 0.0, a_q = 0.0;
        for (int i = threadIdx.x; i < len; i += kDcBlock) {
            const float2 x = in[start + i];
            a_i += (double)x.x;
            a_q += (double)x.y;
        }
        a_i = dc_block_sum(a_i, s_w);
        a_q = dc_block_sum(a_q, s_w);
        if (threadIdx.x == 0) { sums[c] = a_i; sums[n_chunks + c] = a_q; }
    }
}
// guess[col * n_chunks + c] = fl32(sum of the chunk sums in front of c); workgroup `col` of two, 1024 threads with a slice each
__global__ void __launch_bounds__(1024) k_dc_prefix(const double *sums, int64_t n_chunks, float *guess) {
    __shared__ double s_p[1024];
    const double *s = sums + blockIdx.x * n_chunks;
    float *g = guess + blockIdx.x * n_chunks;
    const int64_t per = (n_chunks + 1023) / 1024, lo = std::min<int64_t>(n_chunks, threadIdx.x * per), hi = std::min<int64_t>(n_chunks, lo + per);
    double a = 0.0;
    for (int64_t c = lo; c < hi; ++c) a += s[c];
    s_p[threadIdx.x] = a;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {             // inclusive scan of the slices' sums
        const double add = (int)threadIdx.x >= o ? s_p[threadIdx.x - o] : 0.0;
        __syncthreads();
        s_p[threadIdx.x] += add;
        __syncthreads();
    }
    double run = threadIdx.x ? s_p[threadIdx.x - 1] : 0.0;
    for (int64_t c = lo; c < hi; ++c) { g[c] = (float)run; run += s[c]; }
}

// ---- float32, pass 2: speculation ----------------------------------------------------------------------------------------------------
// Two paths per (chunk, column): from the guess and from its neighbour one ulp further from zero.  Whatever the true entry is, it is an EVEN
// number of ulps from one of the two, and paths an even distance apart make the same choice at every tie: ties cost nothing.
// rec[2 * (2 * c + col) + p] = {entry bits, exit bits, smallest |s| bits, largest |s| bits (all ones: the sign changed)}
struct DcPath {
    float s;
    uint32_t entry, mn, mx, flip;
    __device__ __forceinline__ void begin(uint32_t bits) {
        s = __uint_as_float(bits);
        entry = bits;
        mn = mx = entry & 0x7fffffffu;
        flip = 0;
    }
    __device__ __forceinline__ void step(float x) {
        s += x;
        const uint32_t b = __float_as_uint(s), a = b & 0x7fffffffu;
        mn = std::min(mn, a);
        mx = std::max(mx, a);
        flip |= b ^ entry;
    }
    __device__ __forceinline__ uint4 record() const {
        return make_uint4(entry, __float_as_uint(s), mn, (flip & 0x80000000u) ? 0xffffffffu : mx);
    }
};

__global__ void __launch_bounds__(64) k_dc_spec(const float *__restrict__ in, int64_t n, int64_t n_chunks, const float *guess, uint4 *rec) {
    const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x, c = g >> 1;
    const int col = (int)(g & 1);
    if (c >= n_chunks) return;
    const int64_t start = c * kDcChunk;
    const int len = (int)std::min<int64_t>(kDcChunk, n - start);
    const float *p = in + 2 * start + col;
    DcPath path, odd;
    const uint32_t g_bits = __float_as_uint(guess[col * n_chunks + c]);
    path.begin(g_bits);
    odd.begin(g_bits + 1);
    float cur[kDcSpecBatch], nxt[kDcSpecBatch];
    int base = 0;
    if (len >= kDcSpecBatch) {
#pragma unroll
        for (int k = 0; k < kDcSpecBatch; ++k) cur[k] = p[2 * k];
    }
    for (; base + kDcSpecBatch <= len; base += kDcSpecBatch) {
        const bool more = base + 2 * kDcSpecBatch <= len;
        if (more) {
#pragma unroll
            for (int k = 0; k < kDcSpecBatch; ++k) nxt[k] = p[2 * (base + kDcSpecBatch + k)];
        }
#pragma unroll
        for (int k = 0; k < kDcSpecBatch; ++k) { path.step(cur[k]); odd.step(cur[k]); }
        if (more) {
#pragma unroll
            for (int k = 0; k < kDcSpecBatch; ++k) cur[k] = nxt[k];
        }
    }
    for (; base < len; ++base) { const float x = p[2 * base]; path.step(x); odd.step(x); }
    rec[2 * (2 * c + col)] = path.record();
    rec[2 * (2 * c + col) + 1] = odd.record();
}

// ---- float32, pass 3: stitch ---------------------------------------------------------------------------------------------------------
// The true exit of a chunk entered with the bits `t`, where its two records allow it to be derived; kind: 1 entered as guessed, 2 translated
__device__ __forceinline__ bool dc_derive(const uint4 r0, const uint4 r1, uint32_t &t, int &kind) {
    if (t == r0.x) { t = r0.y; kind = 1; return true; }
    if (t == r1.x) { t = r1.y; kind = 1; return true; }
    if ((t & 0x7fffffffu) > 0x7f800000u) { kind = 2; return true; }        // a NaN sum absorbs whatever follows
    const uint4 r = ((t ^ r0.x) & 1u) ? r1 : r0;                            // the path an even number of ulps away
    if (((t ^ r.x) >> 31) || r.w == 0xffffffffu) return false;
    const uint32_t ga = r.x & 0x7fffffffu, lo = ga & 0x7f800000u, hi = lo | 0x007fffffu;
    const uint32_t mn = r.z, mx = r.w;
    if (lo == 0x7f800000u || mn < lo || mx > hi) return false;
    const long long d = (long long)(t & 0x7fffffffu) - (long long)ga, ad = d < 0 ? -d : d;
    if (ad + 1 > (long long)std::min(mn - lo, hi - mx)) return false;
    t = (r.y & 0x80000000u) | (uint32_t)((long long)(r.y & 0x7fffffffu) + d);
    kind = 2;
    return true;
}

__global__ void __launch_bounds__(64) k_dc_stitch(const float2 *__restrict__ in, int64_t n, int64_t n_chunks, const uint4 *rec, int direct,
                                                  float *mean, float *user_mean, long long *stats) {
    __shared__ uint4 s_rec[128];
    __shared__ float2 s_x[kDcChunk];
    const int lane = threadIdx.x, col = lane & 1;
    uint32_t t = 0;                                   // +0.0: numpy's accumulator starts there
    long long n_same = 0, n_moved = 0, n_redo = 0;
    for (int64_t base = 0; base < n_chunks; base += 32) {
        const int cnt = (int)std::min<int64_t>(32, n_chunks - base);
        if (!direct) {
            if (lane < 4 * cnt) s_rec[lane] = rec[4 * base + lane];
            if (lane + 64 < 4 * cnt) s_rec[lane + 64] = rec[4 * base + lane + 64];
        }
        __syncthreads();
        int j = lane < 2 ? 0 : cnt;
        for (;;) {
            if (lane < 2 && !direct) {
                for (; j < cnt; ++j) {
                    int kind = 0;
                    if (!dc_derive(s_rec[2 * (2 * j + col)], s_rec[2 * (2 * j + col) + 1], t, kind)) break;
                    if (kind == 1) ++n_same; else ++n_moved;
                }
            }
            const int jm = std::min(__shfl(j, 0, 64), __shfl(j, 1, 64));
            if (jm >= cnt) break;
            // a chunk one of the columns cannot derive: into LDS, then that column's lane walks it from its true entry
            const int64_t start = (base + jm) * kDcChunk;
            const int len = (int)std::min<int64_t>(kDcChunk, n - start);
            __syncthreads();
            for (int i = lane; i < len; i += 64) s_x[i] = in[start + i];
            __syncthreads();
            if (lane < 2 && j == jm) {
                float s = __uint_as_float(t);
                const float *x = (const float *)s_x + col;
                for (int i = 0; i < len; ++i) s += x[2 * i];
                t = __float_as_uint(s);
                ++j;
                ++n_redo;
            }
        }
        __syncthreads();
    }
    const long long same_q = __shfl(n_same, 1, 64), moved_q = __shfl(n_moved, 1, 64), redo_q = __shfl(n_redo, 1, 64);
    if (lane < 2) {
        const float m = (float)((double)__uint_as_float(t) / (double)n);     // numpy: the float32 sum divided in float64, rounded once
        mean[col] = m;
        if (user_mean) user_mean[col] = m;
    }
    if (lane == 0) {
        stats[0] = direct ? 0 : n_chunks;
        stats[1] = n_same + same_q + n_moved + moved_q;
        stats[2] = n_redo + redo_q;
        stats[3] = n_same + same_q;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
static DcSpan dc_span(const void *in, const void *out, int64_t n, int comp_bytes) {
    DcSpan sp;
    sp.n = n;
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    const int sample = 2 * comp_bytes;
    if ((a ^ b) & 15) { sp.head = n; sp.nvec = 0; return sp; }              // the two are aligned differently: sample by sample
    sp.head = std::min<int64_t>(n, (int64_t)(((16 - (a & 15)) & 15) / sample));
    sp.nvec = (n - sp.head) * sample / 16;
    return sp;
}
static int dc_grid(const DcSpan &sp) {
    const int64_t work = std::max<int64_t>(sp.nvec, sp.n - sp.nvec);
    return (int)std::min<int64_t>(kDcMaxGrid, std::max<int64_t>(1, (work + kDcBlock - 1) / kDcBlock));
}

template <class T>
static void dc_launch_int(const void *d_in, void *d_out, int64_t n, char *work, void *d_mean, hipStream_t stream) {
    const DcSpan sp = dc_span(d_in, d_out, n, (int)sizeof(T));
    const int grid = dc_grid(sp);
    double *mean = (double *)(work + kDcOffMean);
    k_dc_isum<T><<<grid, kDcBlock, 0, stream>>>((const T *)d_in, sp, (long long *)(work + kDcOffPart), (unsigned int *)(work + kDcOffTicket), mean,
                                                (double *)d_mean);
    k_dc_sub<T, double><<<grid, kDcBlock, 0, stream>>>((const T *)d_in, (T *)d_out, sp, mean);
}

static void dc_launch_f32(const void *d_in, void *d_out, int64_t n, char *work, void *d_mean, hipStream_t stream) {
    const int64_t n_chunks = (n + kDcChunk - 1) / kDcChunk;
    float *mean = (float *)(work + kDcOffMean);
    long long *stats = (long long *)(work + kDcOffStats);
    if (n <= kDcDirectMax) {
        k_dc_stitch<<<1, 64, 0, stream>>>((const float2 *)d_in, n, n_chunks, nullptr, 1, mean, (float *)d_mean, stats);
    } else {
        double *sums = (double *)(work + kDcHeader);
        float *guess = (float *)(sums + 2 * n_chunks);
        uint4 *rec = (uint4 *)(work + kDcHeader + align256((size_t)n_chunks * 24));
        k_dc_chunk_sums<<<(int)std::min<int64_t>(n_chunks, 8 * kDcMaxGrid), kDcBlock, 0, stream>>>((const float2 *)d_in, n, n_chunks, sums);
        k_dc_prefix<<<2, 1024, 0, stream>>>(sums, n_chunks, guess);
        k_dc_spec<<<(int)((2 * n_chunks + 63) / 64), 64, 0, stream>>>((const float *)d_in, n, n_chunks, guess, rec);
        k_dc_stitch<<<1, 64, 0, stream>>>((const float2 *)d_in, n, n_chunks, rec, 0, mean, (float *)d_mean, stats);
    }
    const DcSpan sp = dc_span(d_in, d_out, n, 4);
    k_dc_sub<float, float><<<dc_grid(sp), kDcBlock, 0, stream>>>((const float *)d_in, (float *)d_out, sp, mean);
}

static size_t dc_work_bytes(int64_t n, int dtype) {
    if (dtype != URHGPU_DT_F32 || n <= kDcDirectMax) return kDcHeader;
    const size_t n_chunks = (size_t)((n + kDcChunk - 1) / kDcChunk);
    return kDcHeader + align256(n_chunks * 24) + n_chunks * 64 + 256;
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_dc_correct_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, void *d_out, void *d_mean) {
    if (!ctx || n < 0 || n > (int64_t(1) << 40)) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (n == 0) return URHGPU_OK;
    const int comp = dtype == URHGPU_DT_F32 ? 4 : (dtype == URHGPU_DT_I16 || dtype == URHGPU_DT_U16) ? 2 : 1;
    const size_t bytes = (size_t)n * 2 * comp;
    if (!d_in || !d_out || ((uintptr_t)d_in % (2 * comp)) || ((uintptr_t)d_out % (2 * comp)) || ((uintptr_t)d_mean & 7)) return URHGPU_ERR_ARG;
    if (d_in != d_out && (const char *)d_in < (const char *)d_out + bytes && (const char *)d_out < (const char *)d_in + bytes) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    const size_t need = dc_work_bytes(n, dtype);
    const bool grow = need > ctx->dc_work.cap;
    if (!ctx->ev_dc) URH_HIP(hipEventCreateWithFlags(&ctx->ev_dc, hipEventDisableTiming));
    else if (ctx->dc_stream != ctx->stream && !grow) URH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_dc, 0));
    if (grow) {
        if (ctx->dc_work.base) ++g_dc_host_syncs;                           // (freeing the old area waits for the device)
        URH_TRY(ctx->dc_work.reserve(std::max(2 * need, size_t(1) << 20)));
        URH_HIP(hipMemsetAsync(ctx->dc_work.base, 0, kDcOffPart, ctx->stream));   // the election ticket starts at zero and is left there
    }
    ctx->dc_stream = ctx->stream;
    char *work = (char *)ctx->dc_work.base;
    switch (dtype) {
        case URHGPU_DT_I8: dc_launch_int<int8_t>(d_in, d_out, n, work, d_mean, ctx->stream); break;
        case URHGPU_DT_U8: dc_launch_int<uint8_t>(d_in, d_out, n, work, d_mean, ctx->stream); break;
        case URHGPU_DT_I16: dc_launch_int<int16_t>(d_in, d_out, n, work, d_mean, ctx->stream); break;
        case URHGPU_DT_U16: dc_launch_int<uint16_t>(d_in, d_out, n, work, d_mean, ctx->stream); break;
        default: dc_launch_f32(d_in, d_out, n, work, d_mean, ctx->stream); break;
    }
    URH_HIP(hipGetLastError());
    URH_HIP(hipEventRecord(ctx->ev_dc, ctx->stream));
    return URHGPU_OK;
}

int64_t urhgpu_test_dc_host_syncs(void) { return (int64_t)g_dc_host_syncs.load(); }

int urhgpu_test_dc_stats(urhgpu_ctx *ctx, int64_t *stats) {
    if (!ctx || !stats) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    if (!ctx->dc_work.base) { stats[0] = stats[1] = stats[2] = stats[3] = 0; return URHGPU_OK; }
    URH_HIP(hipMemcpyAsync(stats, (const char *)ctx->dc_work.base + kDcOffStats, 32, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
