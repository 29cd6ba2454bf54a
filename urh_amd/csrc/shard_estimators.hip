// shard_estimators.hip -- the partial reductions behind detect_noise_level and detect_center of a capture that is sharded over
// several GPUs (urh_amd/sharding.py: ShardedPipeline.detect_noise_level / detect_center).  A rank reduces what its own samples
// allow; what is left crosses the ranks in one small all-gather and is finished by a pure host function every rank evaluates.
//
//   urhgpu_magnitude_chunk_partials_dev   detect_noise_level (AutoInterpretation.py:60-91): fp64 sum and max of the magnitudes of
//                                         the intersection of every (global) chunk with the shard
//   urhgpu_pairwise_partial_f32_dev       np.mean / np.var of detect_center (AutoInterpretation.py:226-277): the part of numpy's
//                                         float32 summation tree (pairwise.hpp) that lies inside the rank's elements
//
// Record of urhgpu_pairwise_partial_f32_dev (float32 words; sharding.py reads it, URHGPU_PW_REC_* in include/urhgpu.h):
//     [0:2) g_off, [2:4) m_local as int64        [4] min, [5] max of the rank's elements (+inf / -inf without a non-NaN element),
//     [6] the rank's first element, [7] number of words as int32
//     [8, 136)    head: the elements (mapped through `mode`) of the leaf the range's START cuts, or of a range inside one leaf
//     [136, 264)  leaf sums of the first piece the range touches when it is not wholly inside: the leaf whose first multiple of 64
//     [264, 392)  ... and of the last such piece                       (relative to the piece) is 64 s sits in slot s
//     [392, 520)  tail: the mapped elements of the leaf the range's END cuts
//     [520, ...)  one sum per full piece of 8192 elements wholly inside the range, ascending
// A piece's leaves are 64 .. 128 elements long (a piece of <= 128 elements is one leaf), so every leaf holds exactly one first
// multiple of 64 and the slots are a fixed layout: no ranking, no counts, and a reader that knows (g_off, m_local, m_total) knows
// where everything is.  Unused words are zero.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "common.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"
#include "magnitude.hpp"
#include "pairwise.hpp"

namespace urh {

// ---- detect_noise_level on a shard --------------------------------------------------------------------------------------------
// Chunk k (counted from the END of the capture) = global samples [n_total - (k + 1) chunk, n_total - k chunk).  Workgroup (slice, j)
// reduces the part of slice `slice` of chunk k_first + j that lies in the shard; thread t looks at the global positions
// slice start + t + 256 i, as k_mag_chunk_partials does, so a shard that is the whole capture adds the same terms in the same order.
constexpr int kSpMagSlices = 32;

template <int DT>
__global__ __launch_bounds__(256) void k_sp_mag_partials(const void *iq, int64_t n_local, int64_t pos_base, int64_t n_total, int64_t chunk,
                                                          int64_t k_first, double *part_sum, double *part_max) {
    __shared__ double s_sum[4], s_max[4];
    const int64_t k = k_first + blockIdx.y;
    const int64_t lo = n_total - (k + 1) * chunk, hi = lo + chunk;
    const int64_t L = (chunk + kSpMagSlices - 1) / kSpMagSlices;
    const int64_t a0 = lo + (int64_t)blockIdx.x * L;
    int64_t a1 = (a0 + L < hi) ? a0 + L : hi;
    if (a1 > pos_base + n_local) a1 = pos_base + n_local;
    int64_t i = a0 + threadIdx.x;
    if (i < pos_base) i += (pos_base - i + 255) / 256 * 256;
    double sum = 0.0, mx = 0.0;
    bool any_nan = false;
    for (; i < a1; i += 256) {
        const double v = MagLoad<DT>::mag(iq, i - pos_base);
        sum += v;
        if (v != v) any_nan = true; else mx = (v > mx) ? v : mx;
    }
    if (any_nan) mx = __builtin_nan("");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o);
        const double om = __shfl_down(mx, o);
        mx = (om != om || mx != mx) ? __builtin_nan("") : ((om > mx) ? om : mx);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sum[wave] = sum; s_max[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, tm = 0.0; bool nan = false;
        for (int w = 0; w < 4; ++w) { ts += s_sum[w]; if (s_max[w] != s_max[w]) nan = true; else tm = (s_max[w] > tm) ? s_max[w] : tm; }
        part_sum[(int64_t)blockIdx.y * kSpMagSlices + blockIdx.x] = ts;
        part_max[(int64_t)blockIdx.y * kSpMagSlices + blockIdx.x] = nan ? __builtin_nan("") : tm;
    }
}

__global__ void k_sp_mag_finish(const double *part_sum, const double *part_max, int64_t k_first, int64_t n_touched, double *d_sum, double *d_max) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= n_touched) return;
    double ts = 0.0, tm = 0.0; bool nan = false;
    for (int s = 0; s < kSpMagSlices; ++s) {
        ts += part_sum[j * kSpMagSlices + s];
        const double m = part_max[j * kSpMagSlices + s];
        if (m != m) nan = true; else tm = (m > tm) ? m : tm;
    }
    d_sum[k_first + j] = ts;
    d_max[k_first + j] = nan ? __builtin_nan("") : tm;
}

// the chunks [k_first, k_first + n_touched) that intersect the shard [pos_base, pos_base + n_local)
static void sp_touched_chunks(int64_t n_local, int64_t pos_base, int64_t n_total, int64_t chunk, int64_t n_chunks, int64_t *k_first,
                              int64_t *n_touched) {
    *k_first = 0; *n_touched = 0;
    if (n_local <= 0 || n_chunks <= 0) return;
    const int64_t e = pos_base + n_local;                   // chunk k intersects iff n_total - (k + 1) chunk < e and n_total - k chunk > pos_base
    const int64_t kf = (n_total - e) / chunk;               // smallest k with n_total - (k + 1) chunk < e
    int64_t kl = (n_total - pos_base - 1) / chunk;          // largest k with n_total - k chunk > pos_base
    if (kl > n_chunks - 1) kl = n_chunks - 1;
    if (kl < kf) return;
    *k_first = kf; *n_touched = kl - kf + 1;
}

size_t sp_mag_scratch_bytes(int64_t n_chunks) { return 2 * align256((size_t)std::max<int64_t>(n_chunks, 1) * kSpMagSlices * 8) + 512; }

template <int DT>
static void sp_mag_launch_dt(const void *iq, int64_t n_local, int64_t pos_base, int64_t n_total, int64_t chunk, int64_t kf, int64_t nt,
                             double *ps, double *pm, double *d_sum, double *d_max, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_mag_partials<DT>, dim3(kSpMagSlices, (unsigned)nt), dim3(256), 0, s, iq, n_local, pos_base, n_total, chunk, kf, ps, pm);
    hipLaunchKernelGGL(k_sp_mag_finish, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, ps, pm, kf, nt, d_sum, d_max);
}

int launch_mag_chunk_partials(const void *iq, int dtype, int64_t n_local, int64_t pos_base, int64_t n_total, int64_t chunk, int64_t n_chunks,
                              double *d_sum, double *d_max, void *scratch, hipStream_t s) {
    // chunks without a sample of the shard: 0.0 and 0.0 (all bits zero)
    if (hipMemsetAsync(d_sum, 0, (size_t)n_chunks * 8, s) != hipSuccess || hipMemsetAsync(d_max, 0, (size_t)n_chunks * 8, s) != hipSuccess)
        return URHGPU_ERR_HIP;
    int64_t kf, nt;
    sp_touched_chunks(n_local, pos_base, n_total, chunk, n_chunks, &kf, &nt);
    if (nt == 0) return URHGPU_OK;
    if (nt > 65535) return URHGPU_ERR_ARG;                  // (detect_noise_level's geometry has at most 199 chunks)
    double *ps = (double *)scratch;
    double *pm = (double *)((char *)scratch + align256((size_t)n_chunks * kSpMagSlices * 8));
    return dispatch_dtype(dtype, [&](auto dt) {
        sp_mag_launch_dt<dt.value>(iq, n_local, pos_base, n_total, chunk, kf, nt, ps, pm, d_sum, d_max, s);
        return URHGPU_OK;
    });
}

// ---- numpy's float32 summation tree from an arbitrary global offset ----------------------------------------------------------------
// x holds the elements [g0, g1) of a sequence of m_total; the order is pairwise.hpp's.  Eight lanes per leaf, one per accumulator:
// lane j of a leaf reads its elements j, 8 + j, 16 + j, ... (the access pattern of k_me_leaves, msg_estimators.hip), the three
// shuffles are ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), and lane 0 adds the len % 8 tail in order.  No FMA: the unit is
// built with -ffp-contract=off like every summing kernel (build.py).
constexpr int kSpHead = URHGPU_PW_REC_HEAD, kSpFirst = URHGPU_PW_REC_FIRST, kSpLast = URHGPU_PW_REC_LAST, kSpTail = URHGPU_PW_REC_TAIL,
              kSpPieces = URHGPU_PW_REC_PIECES;
constexpr int kSpEdgeBlock = 1024;            // 128 slots x 8 lanes
constexpr int kSpPieceBlock = 512;            // 64 leaves x 8 lanes

struct SpEdge { int64_t p0; int32_t plen; int32_t active; };      // a piece the range touches without holding all of it: global start, length

__device__ __forceinline__ float sp_map(float v, int mode, float mean) {
    if (mode == 0) return v;
    const float d = v - mean;
    return d * d;
}
// util.minmax's comparisons (a NaN never replaces a value); the seed is the caller's business
__device__ __forceinline__ void sp_fold(float v, float &mn, float &mx) {
    if (v < mn) mn = v;
    if (v > mx) mx = v;
}
// (min, max) of the workgroup -> out[0], out[1]; s_mm: 2 x (threads / 64) floats
__device__ __forceinline__ void sp_block_minmax(float mn, float mx, float *s_mm, float *out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float a = __shfl_down(mn, o), b = __shfl_down(mx, o);
        if (a < mn) mn = a;
        if (b > mx) mx = b;
    }
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mm[threadIdx.x >> 6] = mn; s_mm[nw + (threadIdx.x >> 6)] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) { if (s_mm[w] < mn) mn = s_mm[w]; if (s_mm[nw + w] > mx) mx = s_mm[nw + w]; }
        out[0] = mn; out[1] = mx;
    }
}

// the (at most two) pieces at the ends of the range: leaf sums of the leaves wholly inside, the mapped elements of the cut ones
__global__ __launch_bounds__(kSpEdgeBlock) void k_sp_edges(const float *x, int64_t g0, int64_t g1, SpEdge e0, SpEdge e1, int mode, float mean,
                                                            float *rec, float *mm) {
    __shared__ float s_mm[2 * kSpEdgeBlock / 64];
    const SpEdge e = blockIdx.x ? e1 : e0;
    float mn = INFINITY, mx = -INFINITY;
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int64_t q = 64ll * slot;                        // the slot's multiple of 64, relative to the piece
    int64_t off = 0, len = 0;
    bool own = false;
    if (e.active && q < e.plen) {
        len = e.plen;
        while (len > kPwLeaf) {                           // walk down to the leaf that holds q
            const int64_t n2 = pw_split(len);
            if (q < off + n2) len = n2; else { off += n2; len -= n2; }
        }
        own = (q - off) < 64;                             // q is the leaf's first multiple of 64
    }
    const int64_t l0 = e.p0 + off, l1 = l0 + len;
    const int64_t lo = l0 > g0 ? l0 : g0, hi = l1 < g1 ? l1 : g1;
    const bool whole = own && l0 >= g0 && l1 <= g1;
    const bool cut = own && !whole && lo < hi;
    const float *r = x + (l0 - g0);                       // dereferenced only where the leaf lies inside [g0, g1)
    const int nb = (int)(len - len % 8);
    float acc = 0.f;
    if (whole && len >= 8) {
        float v = r[j];
        sp_fold(v, mn, mx);
        acc = sp_map(v, mode, mean);
        for (int i = 8; i < nb; i += 8) {
            v = r[i + j];
            sp_fold(v, mn, mx);
            acc += sp_map(v, mode, mean);
        }
    }
    acc = acc + __shfl_down(acc, 1);
    acc = acc + __shfl_down(acc, 2);
    acc = acc + __shfl_down(acc, 4);
    if (whole && j == 0) {
        int i = nb;
        if (len < 8) { acc = 0.f; i = 0; }
        for (; i < len; ++i) {
            const float v = r[i];
            sp_fold(v, mn, mx);
            acc += sp_map(v, mode, mean);
        }
        rec[(blockIdx.x ? kSpLast : kSpFirst) + slot] = acc;
    }
    if (cut) {
        float *dst = rec + (l0 < g0 ? kSpHead : kSpTail);     // cut by the range's start (or by both ends): head; by its end only: tail
        for (int64_t i = lo + j; i < hi; i += 8) {
            const float v = x[i - g0];
            sp_fold(v, mn, mx);
            dst[i - lo] = sp_map(v, mode, mean);
        }
    }
    sp_block_minmax(mn, mx, s_mm, mm + 2 * blockIdx.x);
}

// one workgroup per full piece wholly inside the range: 64 leaves, then the perfect tree s[i] = s[2 i] + s[2 i + 1] over them
__global__ __launch_bounds__(kSpPieceBlock) void k_sp_pieces(const float *x, int mode, float mean, float *piece_sums, float *mm) {
    __shared__ float s_mm[2 * kSpPieceBlock / 64];
    __shared__ float s_h[kSpPieceBlock / 64];
    const int j = threadIdx.x & 7;
    const float *r = x + (int64_t)blockIdx.x * kPwChunk + (threadIdx.x >> 3) * kPwLeaf;
    float mn = INFINITY, mx = -INFINITY;
    float v = r[j];
    sp_fold(v, mn, mx);
    float acc = sp_map(v, mode, mean);
#pragma unroll
    for (int i = 8; i < kPwLeaf; i += 8) {
        v = r[i + j];
        sp_fold(v, mn, mx);
        acc += sp_map(v, mode, mean);
    }
    acc = acc + __shfl_down(acc, 1);
    acc = acc + __shfl_down(acc, 2);
    acc = acc + __shfl_down(acc, 4);
    acc = acc + __shfl_down(acc, 8);                      // the wavefront's 8 leaves: three levels of the tree
    acc = acc + __shfl_down(acc, 16);
    acc = acc + __shfl_down(acc, 32);
    if ((threadIdx.x & 63) == 0) s_h[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        piece_sums[blockIdx.x] = ((s_h[0] + s_h[1]) + (s_h[2] + s_h[3])) + ((s_h[4] + s_h[5]) + (s_h[6] + s_h[7]));
    sp_block_minmax(mn, mx, s_mm, mm + 2 * ((int64_t)blockIdx.x + 2));
}

// header of the record; min / max over the n_mm partials of the two kernels above
__global__ __launch_bounds__(256) void k_sp_header(const float *x, int64_t g0, int64_t m_local, const float *mm, int64_t n_mm, int32_t n_words,
                                                    float *rec) {
    __shared__ float s_mm[2 * 256 / 64];
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t b = threadIdx.x; b < n_mm; b += 256) {
        if (mm[2 * b] < mn) mn = mm[2 * b];
        if (mm[2 * b + 1] > mx) mx = mm[2 * b + 1];
    }
    sp_block_minmax(mn, mx, s_mm, rec + 4);
    if (threadIdx.x == 0) {
        int64_t *h = (int64_t *)rec;
        h[0] = g0; h[1] = m_local;
        rec[6] = m_local > 0 ? x[0] : 0.f;
        ((int32_t *)rec)[7] = n_words;
    }
}

// full pieces wholly inside [g0, g0 + m) of a sequence of m_total: [*pa, *pb)
static void sp_inside_pieces(int64_t g0, int64_t m, int64_t m_total, int64_t *pa, int64_t *pb) {
    const int64_t n_full = m_total / kPwChunk;
    *pa = (g0 + kPwChunk - 1) / kPwChunk;
    *pb = std::min((g0 + m) / kPwChunk, n_full);
    if (*pb < *pa) *pb = *pa;
}

int64_t pairwise_partial_words(int64_t m_local, int64_t g_off, int64_t m_total) {
    int64_t pa, pb;
    sp_inside_pieces(g_off, m_local, m_total, &pa, &pb);
    return kSpPieces + (pb - pa);
}

size_t pairwise_partial_scratch_bytes(int64_t m_local) { return (size_t)(m_local / kPwChunk + 4) * 8 + 256; }

int launch_pairwise_partial(const float *x, int64_t m_local, int64_t g_off, int64_t m_total, int mode, float mean, float *rec, void *scratch,
                            hipStream_t s) {
    int64_t pa, pb;
    sp_inside_pieces(g_off, m_local, m_total, &pa, &pb);
    const int64_t n_in = pb - pa, g1 = g_off + m_local;
    if (hipMemsetAsync(rec, 0, (size_t)kSpPieces * 4, s) != hipSuccess) return URHGPU_ERR_HIP;
    float *mm = (float *)scratch;
    int64_t n_mm = 0;
    if (m_local > 0) {
        const int64_t n_full = m_total / kPwChunk, p_first = g_off / kPwChunk, p_last = (g1 - 1) / kPwChunk;
        auto edge = [&](int64_t p, bool on) {
            SpEdge e;
            e.p0 = p * kPwChunk;
            e.plen = (int32_t)(p < n_full ? kPwChunk : m_total - n_full * kPwChunk);
            e.active = (on && !(p >= pa && p < pb)) ? 1 : 0;
            return e;
        };
        const SpEdge e0 = edge(p_first, true), e1 = edge(p_last, p_last != p_first);
        hipLaunchKernelGGL(k_sp_edges, dim3(2), dim3(kSpEdgeBlock), 0, s, x, g_off, g1, e0, e1, mode, mean, rec, mm);
        if (n_in > 0)
            hipLaunchKernelGGL(k_sp_pieces, dim3((unsigned)n_in), dim3(kSpPieceBlock), 0, s, x + (pa * kPwChunk - g_off), mode, mean, rec + kSpPieces,
                               mm);
        n_mm = n_in + 2;
    }
    hipLaunchKernelGGL(k_sp_header, dim3(1), dim3(256), 0, s, x, g_off, m_local, mm, n_mm, (int32_t)(kSpPieces + n_in), rec);
    return URHGPU_OK;
}

}  // namespace urh
