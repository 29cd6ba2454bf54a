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
//
// Sharded captures (urhgpu_shard_dc_*_dev, at the end of this file): a rank evaluates its shard of the recurrence with the same chunks from two
// guessed entries, records per column and path {entry, exit, room} -- `room`: by how many ulps (an even number) the entry may move such that every
// chunk is still derived by the record that derived it -- and, where the gathered records do not reach, stitches again from its true entry.
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "dc_sub.hpp"
#include "dispatch.hpp"

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
constexpr size_t kDcOffShardStats = 160;             // int64[8]: the shard's speculation, the shard's resolve
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
                                                       double *user_mean, long long *words) {
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
        if (words) {                                 // a shard: the count and the exact sums, for the mean of the whole capture
            words[0] = sp.n; words[1] = sum_i; words[2] = sum_q;
        } else {
            const double m_i = (double)sum_i / (double)sp.n, m_q = (double)sum_q / (double)sp.n;
            mean[0] = m_i; mean[1] = m_q;
            if (user_mean) { user_mean[0] = m_i; user_mean[1] = m_q; }
        }
        *ticket = 0;                                 // the next call's election
    }
}

// ---- the subtraction, every sample type (dc_sub: dc_sub.hpp) -------------------------------------------------------------------------
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
                                                (double *)d_mean, nullptr);
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

// the context's work area with room for `need` bytes, behind whatever used it last (on another stream: ev_dc)
static int dc_work_area(urhgpu_ctx *ctx, size_t need) {
    URH_HIP(hipSetDevice(ctx->device));
    const bool grow = need > ctx->dc_work.cap;
    if (!ctx->ev_dc) URH_HIP(hipEventCreateWithFlags(&ctx->ev_dc, hipEventDisableTiming));
    else if (ctx->dc_stream != ctx->stream && !grow) URH_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_dc, 0));
    if (grow) {
        if (ctx->dc_work.base) ++g_dc_host_syncs;                           // (freeing the old area waits for the device)
        URH_TRY(ctx->dc_work.reserve(std::max(2 * need, size_t(1) << 20)));
        URH_HIP(hipMemsetAsync(ctx->dc_work.base, 0, kDcOffPart, ctx->stream));   // the election ticket starts at zero and is left there
    }
    ctx->dc_stream = ctx->stream;
    return URHGPU_OK;
}

static size_t dc_work_bytes(int64_t n, int dtype) {
    if (dtype != URHGPU_DT_F32 || n <= kDcDirectMax) return kDcHeader;
    const size_t n_chunks = (size_t)((n + kDcChunk - 1) / kDcChunk);
    return kDcHeader + align256(n_chunks * 24) + n_chunks * 64 + 256;
}


// ---- sharded captures ----------------------------------------------------------------------------------------------------------------
// A shard is always evaluated in chunks (one chunk at least, however short): its records are what the other ranks get.
constexpr uint32_t kDcRoomMax = 0x7ffffffeu;
constexpr uint32_t kDcIdentity = 1u;                 // record flag: the shard holds no sample

// k_dc_prefix with a base: guess[col * n_chunks + c] = fl32(base[col] + the sum of the chunk sums in front of c); words (may be nullptr) =
// {n, the bits of the two float64 sums of all chunks}
__global__ void __launch_bounds__(1024) k_dc_prefix_base(const double *sums, int64_t n_chunks, double base_i, double base_q, float *guess, long long *words,
                                                         long long n) {
    __shared__ double s_p[1024];
    const double *s = sums + blockIdx.x * n_chunks;
    const double b = blockIdx.x ? base_q : base_i;
    const int64_t per = (n_chunks + 1023) / 1024, lo = std::min<int64_t>(n_chunks, threadIdx.x * per), hi = std::min<int64_t>(n_chunks, lo + per);
    double a = 0.0;
    for (int64_t c = lo; c < hi; ++c) a += s[c];
    s_p[threadIdx.x] = a;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const double add = (int)threadIdx.x >= o ? s_p[threadIdx.x - o] : 0.0;
        __syncthreads();
        s_p[threadIdx.x] += add;
        __syncthreads();
    }
    if (guess) {
        float *g = guess + blockIdx.x * n_chunks;
        double run = threadIdx.x ? s_p[threadIdx.x - 1] : 0.0;
        for (int64_t c = lo; c < hi; ++c) { g[c] = (float)(b + run); run += s[c]; }
    }
    if (words && threadIdx.x == 1023) {
        words[1 + blockIdx.x] = __double_as_longlong(s_p[1023]);
        if (blockIdx.x == 0) words[0] = n;
    }
}

// dc_derive that also takes the chunk's share of the shard's room: m - 1 - |d| where the chunk is derived from a record whose path keeps m ulps
// from its binade's edges and was entered d ulps from that record's entry; nothing where the record cannot be translated or the sum is NaN
__device__ __forceinline__ bool dc_derive_room(const uint4 r0, const uint4 r1, uint32_t &t, uint32_t &room) {
    const bool hit0 = t == r0.x, hit = hit0 || t == r1.x;
    if (!hit && (t & 0x7fffffffu) > 0x7f800000u) { room = 0; return true; }
    const uint4 r = hit ? (hit0 ? r0 : r1) : (((t ^ r0.x) & 1u) ? r1 : r0);
    const uint32_t ga = r.x & 0x7fffffffu, lo = ga & 0x7f800000u, hi = lo | 0x007fffffu;
    long long m = -1;
    if (!((t ^ r.x) >> 31) && r.w != 0xffffffffu && lo != 0x7f800000u && r.z >= lo && r.w <= hi) m = (long long)std::min(r.z - lo, hi - r.w);
    const long long d = (long long)(t & 0x7fffffffu) - (long long)ga, ad = d < 0 ? -d : d;
    if (hit) {
        t = r.y;
        room = (uint32_t)std::min<long long>(room, std::max<long long>(m - 1, 0));
        return true;
    }
    if (m < 0 || ad + 1 > m) return false;
    t = (r.y & 0x80000000u) | (uint32_t)((long long)(r.y & 0x7fffffffu) + d);
    room = (uint32_t)std::min<long long>(room, m - 1 - ad);
    return true;
}

struct DcEntries {
    uint32_t e[6];                                   // [2 * path + column]
};
// One wavefront stitches the shard from up to three entries per column at once (lane = 2 * path + column), as k_dc_stitch does from +0.0.
// out_rec (speculation): rec[2 * column + path] = {entry, exit, room, flags}; out_exit (resolve, one path): the two exits.
__global__ void __launch_bounds__(64) k_dc_shard_stitch(const float2 *__restrict__ in, int64_t n, int64_t n_chunks, const uint4 *rec, DcEntries ent, int n_paths,
                                                        uint4 *out_rec, uint32_t *out_exit, long long *stats) {
    __shared__ uint4 s_rec[128];
    __shared__ float2 s_x[kDcChunk];
    const int lane = threadIdx.x, col = lane & 1;
    const bool active = lane < 2 * n_paths;
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) if (lane == k) t = ent.e[k];
    const uint32_t entry = t;
    uint32_t room = kDcRoomMax;
    long long n_derived = 0, n_redo = 0;
    for (int64_t base = 0; base < n_chunks; base += 32) {
        const int cnt = (int)std::min<int64_t>(32, n_chunks - base);
        if (lane < 4 * cnt) s_rec[lane] = rec[4 * base + lane];
        if (lane + 64 < 4 * cnt) s_rec[lane + 64] = rec[4 * base + lane + 64];
        __syncthreads();
        int j = active ? 0 : cnt;
        for (;;) {
            if (active) {
                for (; j < cnt; ++j) {
                    if (!dc_derive_room(s_rec[2 * (2 * j + col)], s_rec[2 * (2 * j + col) + 1], t, room)) break;
                    ++n_derived;
                }
            }
            int jm = j;
            for (int o = 32; o > 0; o >>= 1) jm = std::min(jm, __shfl_xor(jm, o, 64));
            if (jm >= cnt) break;
            // a chunk some path cannot derive: into LDS, then the lanes that stand at it walk it from their true entries
            const int64_t start = (base + jm) * kDcChunk;
            const int len = (int)std::min<int64_t>(kDcChunk, n - start);
            __syncthreads();
            for (int i = lane; i < len; i += 64) s_x[i] = in[start + i];
            __syncthreads();
            if (active && j == jm) {
                float s = __uint_as_float(t);
                const float *x = (const float *)s_x + col;
                for (int i = 0; i < len; ++i) s += x[2 * i];
                t = __float_as_uint(s);
                room = 0;
                ++j;
                ++n_redo;
            }
        }
        __syncthreads();
    }
    n_derived = dc_wave_sum(n_derived);
    n_redo = dc_wave_sum(n_redo);
    if (active) {
        if (out_rec) out_rec[2 * col + (lane >> 1)] = make_uint4(entry, t, room & ~1u, n_chunks == 0 ? kDcIdentity : 0u);
        if (out_exit && lane < 2) out_exit[col] = t;
    }
    if (lane == 0) {
        long long *st = stats + (out_rec ? 0 : 4);
        st[0] = n_chunks; st[1] = n_derived; st[2] = n_redo; st[3] = n_paths;
        if (out_rec) stats[4] = stats[5] = stats[6] = stats[7] = 0;
    }
}

template <class M> __global__ void k_dc_put_mean(M *mean, M m_i, M m_q) {
    mean[0] = m_i;
    mean[1] = m_q;
}

static size_t dc_shard_work_bytes(int64_t n) {
    const size_t n_chunks = (size_t)((n + kDcChunk - 1) / kDcChunk);
    return kDcHeader + align256(n_chunks * 24) + n_chunks * 64 + 256;
}
struct DcShardArea {
    int64_t n_chunks;
    double *sums;
    float *guess;
    uint4 *rec;
};
static DcShardArea dc_shard_area(char *work, int64_t n) {
    DcShardArea a;
    a.n_chunks = (n + kDcChunk - 1) / kDcChunk;
    a.sums = (double *)(work + kDcHeader);
    a.guess = (float *)(a.sums + 2 * a.n_chunks);
    a.rec = (uint4 *)(work + kDcHeader + align256((size_t)a.n_chunks * 24));
    return a;
}
static int dc_comp_bytes(int dtype) { return dtype == URHGPU_DT_F32 ? 4 : (dtype == URHGPU_DT_I16 || dtype == URHGPU_DT_U16) ? 2 : 1; }
// a shard argument: n samples of `comp`-byte components at d, aligned to one sample
static bool dc_shard_arg(const void *d, int64_t n, int comp) {
    return n >= 0 && n <= (int64_t(1) << 40) && (n == 0 || (d && (uintptr_t)d % (2 * comp) == 0));
}

template <class T>
static void dc_launch_isum_shard(const void *d_in, int64_t n, char *work, long long *words, hipStream_t stream) {
    const DcSpan sp = dc_span(d_in, d_in, n, (int)sizeof(T));
    k_dc_isum<T><<<dc_grid(sp), kDcBlock, 0, stream>>>((const T *)d_in, sp, (long long *)(work + kDcOffPart), (unsigned int *)(work + kDcOffTicket), nullptr, nullptr,
                                                       words);
}
template <class T, class M>
static void dc_launch_apply(const void *d_in, void *d_out, int64_t n, char *work, const void *h_mean, hipStream_t stream) {
    M *mean = (M *)(work + kDcOffMean);
    const M *m = (const M *)h_mean;
    k_dc_put_mean<M><<<1, 1, 0, stream>>>(mean, m[0], m[1]);
    const DcSpan sp = dc_span(d_in, d_out, n, (int)sizeof(T));
    k_dc_sub<T, M><<<dc_grid(sp), kDcBlock, 0, stream>>>((const T *)d_in, (T *)d_out, sp, mean);
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
    URH_TRY(dc_work_area(ctx, dc_work_bytes(n, dtype)));
    ctx->dc_shard_n = -1;                                                   // (a shard's chunk records are overwritten)
    char *work = (char *)ctx->dc_work.base;
    URH_TRY(dispatch_dtype(dtype, [&](auto dt) {           // (the range check above has refused every other code)
        if constexpr (dt.value == URHGPU_DT_F32) dc_launch_f32(d_in, d_out, n, work, d_mean, ctx->stream);
        else dc_launch_int<typename decltype(dt)::type>(d_in, d_out, n, work, d_mean, ctx->stream);
        return URHGPU_OK;
    }));
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

int urhgpu_shard_dc_sums_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, void *d_words) {
    if (!ctx || !d_words || ((uintptr_t)d_words & 7)) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (!dc_shard_arg(d_in, n, dc_comp_bytes(dtype))) return URHGPU_ERR_ARG;
    URH_TRY(dc_work_area(ctx, dtype == URHGPU_DT_F32 ? dc_shard_work_bytes(n) : kDcHeader));
    ctx->dc_shard_n = -1;
    char *work = (char *)ctx->dc_work.base;
    long long *words = (long long *)d_words;
    if (n == 0) {
        URH_HIP(hipMemsetAsync(d_words, 0, 24, ctx->stream));
    } else {
        URH_TRY(dispatch_dtype(dtype, [&](auto dt) {       // (the range check above has refused every other code)
            if constexpr (dt.value == URHGPU_DT_F32) {
                const DcShardArea a = dc_shard_area(work, n);
                k_dc_chunk_sums<<<(int)std::min<int64_t>(a.n_chunks, 8 * kDcMaxGrid), kDcBlock, 0, ctx->stream>>>((const float2 *)d_in, n, a.n_chunks, a.sums);
                k_dc_prefix_base<<<2, 1024, 0, ctx->stream>>>(a.sums, a.n_chunks, 0.0, 0.0, nullptr, words, n);
            } else
                dc_launch_isum_shard<typename decltype(dt)::type>(d_in, n, work, words, ctx->stream);
            return URHGPU_OK;
        }));
    }
    URH_HIP(hipGetLastError());
    URH_HIP(hipEventRecord(ctx->ev_dc, ctx->stream));
    return URHGPU_OK;
}

int urhgpu_shard_dc_spec_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, const double *base, void *d_records) {
    if (!ctx || !base || !d_records || ((uintptr_t)d_records & 15) || !dc_shard_arg(d_in, n, 4)) return URHGPU_ERR_ARG;
    URH_TRY(dc_work_area(ctx, dc_shard_work_bytes(n)));
    char *work = (char *)ctx->dc_work.base;
    const DcShardArea a = dc_shard_area(work, n);
    DcEntries ent = {};
    for (int col = 0; col < 2; ++col) {
        const float g = (float)base[col];
        uint32_t bits;
        __builtin_memcpy(&bits, &g, 4);
        ent.e[col] = bits;                                                  // the guess ...
        ent.e[2 + col] = bits + 1;                                          // ... and its neighbour one ulp further from zero
    }
    if (n > 0) {
        k_dc_chunk_sums<<<(int)std::min<int64_t>(a.n_chunks, 8 * kDcMaxGrid), kDcBlock, 0, ctx->stream>>>((const float2 *)d_in, n, a.n_chunks, a.sums);
        k_dc_prefix_base<<<2, 1024, 0, ctx->stream>>>(a.sums, a.n_chunks, base[0], base[1], a.guess, nullptr, n);
        k_dc_spec<<<(int)((2 * a.n_chunks + 63) / 64), 64, 0, ctx->stream>>>((const float *)d_in, n, a.n_chunks, a.guess, a.rec);
    }
    k_dc_shard_stitch<<<1, 64, 0, ctx->stream>>>((const float2 *)d_in, n, a.n_chunks, a.rec, ent, 2, (uint4 *)d_records, nullptr,
                                                 (long long *)(work + kDcOffShardStats));
    URH_HIP(hipGetLastError());
    URH_HIP(hipEventRecord(ctx->ev_dc, ctx->stream));
    ctx->dc_shard_in = d_in;
    ctx->dc_shard_n = n;
    return URHGPU_OK;
}

int urhgpu_shard_dc_resolve_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, const uint32_t *entry, void *d_exit) {
    if (!ctx || !entry || !d_exit || ((uintptr_t)d_exit & 7) || !dc_shard_arg(d_in, n, 4)) return URHGPU_ERR_ARG;
    if (ctx->dc_shard_n != n || ctx->dc_shard_in != d_in || dc_shard_work_bytes(n) > ctx->dc_work.cap) return URHGPU_ERR_ARG;   // not the shard last speculated
    URH_TRY(dc_work_area(ctx, dc_shard_work_bytes(n)));
    char *work = (char *)ctx->dc_work.base;
    const DcShardArea a = dc_shard_area(work, n);
    DcEntries ent = {};
    ent.e[0] = entry[0];
    ent.e[1] = entry[1];
    k_dc_shard_stitch<<<1, 64, 0, ctx->stream>>>((const float2 *)d_in, n, a.n_chunks, a.rec, ent, 1, nullptr, (uint32_t *)d_exit,
                                                 (long long *)(work + kDcOffShardStats));
    URH_HIP(hipGetLastError());
    URH_HIP(hipEventRecord(ctx->ev_dc, ctx->stream));
    return URHGPU_OK;
}

int urhgpu_shard_dc_apply_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, const void *mean, void *d_out) {
    if (!ctx || !mean) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    const int comp = dc_comp_bytes(dtype);
    if (!dc_shard_arg(d_in, n, comp) || !dc_shard_arg(d_out, n, comp)) return URHGPU_ERR_ARG;
    if (n == 0) return URHGPU_OK;
    const size_t bytes = (size_t)n * 2 * comp;
    if (d_in != d_out && (const char *)d_in < (const char *)d_out + bytes && (const char *)d_out < (const char *)d_in + bytes) return URHGPU_ERR_ARG;
    URH_TRY(dc_work_area(ctx, kDcHeader));
    char *work = (char *)ctx->dc_work.base;
    URH_TRY(dispatch_dtype(dtype, [&](auto dt) {           // (the range check above has refused every other code)
        using T = typename decltype(dt)::type;             // an integer capture's mean is a pair of doubles, a float32 capture's a pair of floats
        dc_launch_apply<T, std::conditional_t<dt.value == URHGPU_DT_F32, float, double>>(d_in, d_out, n, work, mean, ctx->stream);
        return URHGPU_OK;
    }));
    URH_HIP(hipGetLastError());
    URH_HIP(hipEventRecord(ctx->ev_dc, ctx->stream));
    return URHGPU_OK;
}

int urhgpu_shard_dc_stats(urhgpu_ctx *ctx, int64_t *stats) {
    if (!ctx || !stats) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    if (!ctx->dc_work.base) { for (int k = 0; k < 8; ++k) stats[k] = 0; return URHGPU_OK; }
    URH_HIP(hipMemcpyAsync(stats, (const char *)ctx->dc_work.base + kDcOffShardStats, 64, hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
