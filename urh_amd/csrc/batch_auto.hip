// batch_auto.hip -- a batch of captures, each gated with its OWN automatic noise threshold (include/urhgpu.h "a batch of captures: automatic
// noise threshold per capture").  The reference opens every file of a recording session with detect_noise_level(magnitudes) and demodulates
// with that capture's noise floor (Signal.py:97-103, AutoInterpretation.py:60-91); here K noise floors are decided by ONE launch and the
// batch's walk gates each capture with its own:
//   k_batch_noise<DT>   a workgroup of 256 threads per capture: the per-chunk (sum, max) of the magnitudes -- wavefront w takes chunks w, w + 4,
//                       ... --, then one thread decides with the body k_noise_decide uses (noise_decide.hpp) and stores the capture's
//                       urhgpu_noise_result.
//   k_batch_bits<DT, MOD, ORDER2, true>   batch_kernels.hpp's walk reading noise_sqrd and flag from the capture's block (flag 2: walked as a
//                       capture of two samples -- the reference then slices zeros(2)).
// A chunk's SUM is taken in numpy's float64 pairwise order (pairwise.hpp), so that sum / chunk IS np.mean(chunk) bit for bit: the chunk is
// walked in pieces of kPwChunk terms, total = ((0 + pw(piece 0)) + pw(piece 1)) + ...; a piece splits by pw_split down to leaves of at most
// kPwLeaf terms.  All chunks of a capture have the same length, so the tree is the same for all of them: thread 0 walks it ONCE per workgroup
// and leaves, for a full piece and for the chunk's last piece, the list of leaves (offset, length) and the postfix sequence of additions
// in LDS.  Per piece a wavefront then takes eight leaves at a time, eight lanes per leaf: lane (g, j) adds the terms j, j + 8, ... of leaf g
// in order (at most 16 adds), an xor butterfly over lane distances 1, 2, 4 combines the eight accumulators -- ((r0 + r1) + (r2 + r3)) +
// ((r4 + r5) + (r6 + r7)) in every lane: IEEE addition commutes --, lane (g, 0) adds the leaf's n % 8 tail in order, and lane 0 runs the
// additions on a value stack.  A leaf below 8 terms (a chunk below 8 samples) is summed in order.  The maximum follows np.max: a NaN wins.
// Every term is formed by MagLoad<DT>::mag from global memory when it is added (each is used once) at an index inside the capture: the
// chunks count from the capture's END and the front remainder is never read.  No atomics, nothing waits for another workgroup.
#include "batch_kernels.hpp"      // (first: the fp64 forms of URH_FDIV / URH_FSQRT)

#include <algorithm>

#include "magnitude.hpp"
#include "noise_decide.hpp"
#include "pairwise.hpp"

namespace urh {

// a piece of at most kPwChunk terms: every leaf that comes from a split has at least 64 terms, and a sibling of a 64-term leaf has more
constexpr int kBnLeaves = 128, kBnOps = 2 * kBnLeaves, kBnFrames = 16, kBnVals = 16;
struct BnPlan {
    int n_leaves, n_ops;
    uint16_t off[kBnLeaves];       // a leaf's first term, counted from the piece's
    uint8_t len[kBnLeaves];        // 1 .. kPwLeaf terms
    uint8_t ops[kBnOps];           // postfix: 0 = push the next leaf's sum, 1 = pop b, pop a, push a + b
};
struct BnFrames { int off[kBnFrames], len[kBnFrames], stage[kBnFrames]; };

// pw's tree over `len` terms, depth first (msg_records.hip has the same walk): one thread, its stack in LDS
__device__ __forceinline__ void bn_plan(int len, BnPlan &P, BnFrames &f) {
    int sp = 1, nl = 0, no = 0;
    f.off[0] = 0; f.len[0] = len; f.stage[0] = 0;
    while (sp > 0 && no < kBnOps) {
        const int off = f.off[sp - 1], l = f.len[sp - 1], st = f.stage[sp - 1];
        if (l <= kPwLeaf) {
            if (nl >= kBnLeaves) break;                    // (cannot happen: see kBnLeaves)
            P.off[nl] = (uint16_t)off; P.len[nl] = (uint8_t)l; ++nl;
            P.ops[no++] = 0; --sp;
        } else if (st == 2) {
            P.ops[no++] = 1; --sp;
        } else {
            if (sp >= kBnFrames) break;                    // (cannot happen: a length halves per level, 8192 terms are 7 levels)
            const int n2 = (int)pw_split(l);
            f.stage[sp - 1] = st + 1;
            f.off[sp] = st == 0 ? off : off + n2;
            f.len[sp] = st == 0 ? n2 : l - n2;
            f.stage[sp] = 0;
            ++sp;
        }
    }
    P.n_leaves = nl; P.n_ops = no;
}

template <int DT>
__global__ __launch_bounds__(256) void k_batch_noise(const BatchArgs b, double max_mag, float cfg_noise, urhgpu_noise_result *d_noise) {
    __shared__ double s_sum[kNoiseMaxChunks + 1], s_mx[kNoiseMaxChunks + 1];
    __shared__ float s_mean[kNoiseMaxChunks + 1];
    __shared__ double s_leaf[4][kBnLeaves];
    __shared__ double s_val[4][kBnVals];
    __shared__ BnPlan s_plan[2];                           // 0: a full piece of kPwChunk terms, 1: the chunk's last piece
    __shared__ BnFrames s_frames;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    if ((int64_t)blockIdx.x >= b.k) return;
    const int64_t c = b.plan[2 * b.k + blockIdx.x];        // launch order: longest capture first
    if (c < 0 || c >= b.k) return;
    const BatchCapture cap = batch_capture(b, c);          // (a start or an end that is refused: n = 0, nothing is read)
    const int64_t n = cap.n;
    int64_t chunk = 1;
    int n_chunks = 0;
    if (n > 3) {                                           // :61-72 (int(n * 1 / 100); the front remainder is dropped)
        chunk = n / 100 > 1 ? n / 100 : 1;
        n_chunks = (int)(n / chunk);                       // <= 199
        if (n_chunks > kNoiseMaxChunks) n_chunks = kNoiseMaxChunks;
    }
    const int64_t full = chunk / kPwChunk;
    const int rest = (int)(chunk % kPwChunk);
    if (tid == 0 && n_chunks > 0) {
        if (full > 0) bn_plan(kPwChunk, s_plan[0], s_frames);
        if (rest > 0) bn_plan(rest, s_plan[1], s_frames);
    }
    __syncthreads();
    // every loop bound below is the same for the whole workgroup: the barriers are reached by all four wavefronts
    const int rounds = (n_chunks + 3) / 4;
    for (int r = 0; r < rounds; ++r) {
        const int j = 4 * r + w;
        const bool active = j < n_chunks;
        const int64_t lo = cap.s0 + n - (int64_t)(j + 1) * chunk;       // chunk j = samples [n - (j + 1) chunk, n - j chunk) of THIS capture
        double total = 0.0, mx = 0.0;
        bool nan = false;
#define BN_TERM(i_) MagLoad<DT>::mag(b.iq, (i_)); if (v != v) nan = true; else mx = (v > mx) ? v : mx
        for (int64_t pc = 0; pc <= full; ++pc) {
            const bool last = pc == full;
            if (last && rest == 0) break;
            const BnPlan &P = s_plan[last ? 1 : 0];
            const int64_t pbase = lo + pc * kPwChunk;
            const int nl = P.n_leaves;
            for (int g0 = 0; g0 < nl; g0 += 8) {
                const int g = g0 + (lane >> 3), jj = lane & 7;
                const bool mine = active && g < nl;
                double acc = 0.0;
                int len = 0, m8 = 0;
                int64_t at = 0;
                if (mine) {
                    at = pbase + P.off[g]; len = P.len[g];
                    if (len >= 8) {
                        m8 = len - (len & 7);
                        { const double v = BN_TERM(at + jj); acc = v; }
                        for (int i = 8 + jj; i < m8; i += 8) { const double v = BN_TERM(at + i); acc += v; }
                    }
                }
                acc += __shfl_xor(acc, 1);
                acc += __shfl_xor(acc, 2);
                acc += __shfl_xor(acc, 4);
                if (mine && jj == 0) {
                    double res = len >= 8 ? acc : 0.0;
                    for (int i = m8; i < len; ++i) { const double v = BN_TERM(at + i); res += v; }
                    s_leaf[w][g] = res;
                }
            }
            __syncthreads();
            if (active && lane == 0) {
                int vsp = 0, leaf = 0;
                const int no = P.n_ops;
                for (int o = 0; o < no; ++o) {
                    if (P.ops[o] == 0) { if (vsp < kBnVals) s_val[w][vsp] = s_leaf[w][leaf]; ++vsp; ++leaf; }
                    else if (vsp >= 2 && vsp <= kBnVals) { const double y = s_val[w][vsp - 1], x = s_val[w][vsp - 2]; s_val[w][vsp - 2] = x + y; --vsp; }
                }
                total = total + s_val[w][0];
            }
            __syncthreads();                               // (s_leaf is the next piece's)
        }
#undef BN_TERM
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const double om = __shfl_xor(mx, o); mx = (om > mx) ? om : mx; }
        const bool any_nan = __builtin_amdgcn_ballot_w64(nan) != 0ull;
        if (active && lane == 0) { s_sum[j] = total; s_mx[j] = any_nan ? __builtin_nan("") : mx; }
    }
    __syncthreads();
    if (tid < n_chunks) s_mean[tid] = (float)(s_sum[tid] / (double)chunk);
    __syncthreads();
    if (tid != 0) return;
    d_noise[c] = noise_decide(s_mean, s_mx, chunk, n_chunks, max_mag, cfg_noise, 1);
}

static int launch_batch_noise(const BatchArgs &b, int dtype, double max_mag, float cfg, urhgpu_noise_result *d_noise, unsigned grid, hipStream_t s) {
    return dispatch_dtype(dtype, [&](auto dt) {
        hipLaunchKernelGGL(k_batch_noise<dt.value>, dim3(grid), dim3(256), 0, s, b, max_mag, cfg, d_noise);
        return URHGPU_OK;
    });
}

static int launch_batch_bits_dn(const RunArgs &a, const BatchArgs &b, int dtype, int mod, unsigned grid, hipStream_t s) {
    return dispatch_dtype(dtype, [&](auto dt) {
        return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
            return dispatch_bool(a.order == 2, [&](auto o2) {
                hipLaunchKernelGGL((k_batch_bits<dt.value, m.value, o2.value, true>), dim3(grid), dim3(64), 0, s, a, b);
                return URHGPU_OK;
            });
        });
    });
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_noise_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                           const urhgpu_params *p, urhgpu_noise_result *d_noise) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0) return URHGPU_ERR_ARG;
    URH_TRY(batch_check_params(p));
    if (k > 0 && (!d_start || !d_plan || !d_noise)) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    BatchArgs b;
    memset(&b, 0, sizeof(b));                              // no work buffer: batch_capture then vouches for the samples alone
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total;
    b.sps = p->samples_per_symbol; b.bps = p->bits_per_symbol; b.tol = p->tolerance;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    URH_TRY(launch_batch_noise(b, p->dtype, urhgpu_noise_max_magnitude(p->dtype), p->noise_threshold, d_noise, grid, ctx->stream));
    ctx->batch_launches += 1;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_iq_to_bits_batch_auto_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                     const urhgpu_params *p, float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir,
                                     void *d_blob, int64_t cap_blob, urhgpu_noise_result *d_noise) {
    if ((k > 0 && !d_noise) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    RunArgs a;
    BatchArgs b;
    URH_TRY(batch_setup(ctx, d_iq, total, d_start, d_plan, k, p, d_qad, d_work, work_bytes, d_counts, d_dir, d_blob, cap_blob, a, b));
    a.d_noise = (const float *)d_noise;                    // (k_batch_bits<..., DNOISE>: the base of the K result blocks)
    // four launches whatever k and the lengths are (k = 0: grids of one workgroup that finds nothing to do)
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    URH_TRY(launch_batch_noise(b, p->dtype, urhgpu_noise_max_magnitude(p->dtype), p->noise_threshold, d_noise, grid, ctx->stream));
    ctx->batch_launches += 1;
    URH_TRY(launch_batch_bits_dn(a, b, p->dtype, p->mod, grid, ctx->stream));
    launch_batch_scan_pack(b, grid, ctx->stream);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_noise_fetch(urhgpu_ctx *ctx, const urhgpu_noise_result *d_noise, int64_t k, urhgpu_noise_result *h_noise) {
    if (!ctx || k < 0 || (k > 0 && (!d_noise || !h_noise))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    if (k > 0) {
        URH_HIP(hipMemcpyAsync(h_noise, d_noise, (size_t)k * sizeof(urhgpu_noise_result), hipMemcpyDeviceToHost, ctx->stream));
        ++ctx->batch_copies;
    }
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
