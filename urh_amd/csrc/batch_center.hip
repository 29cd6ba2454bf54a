// batch_center.hip -- a batch of captures, each sliced with its OWN automatic center (include/urhgpu.h "a batch of captures: automatic
// center per capture").  The reference detects the center of every signal it demodulates (AutoInterpretation.detect_center,
// AutoInterpretation.py:226-277), and for ASK the center follows the received amplitude: the captures of a session, tens of dB apart in
// gain, cannot share one.  A pass over the batch:
//   k_batch_noise<DT>               (automatic noise only; batch_auto.hip's launch, urhgpu_batch_noise_dev) a noise floor per capture
//   k_batch_demod<DT, MOD, DNOISE>  a WORKGROUP per capture -- the demodulation has no serial dependency -- strides over the capture's samples
//                                   with coalesced loads and leaves afp_demod's signal of all captures in qad[total]
//   the center chain                msg_estimators.hip: detect_center of the K ranges, states built on the device, never waited for; in
//                                   groups of captures whose histogram pool stays within 64 MiB
//   k_batch_center_publish          a wavefront per capture: its slicing thresholds, its result block, and -- where the second and third
//                                   peak tie -- its histogram's counts appended to a pool for the host
//   k_batch_bits<.., QIN>           batch_kernels.hpp's walk reading qad and classifying through the capture's thresholds
//   k_batch_scan, k_batch_pack      batch.hip's
// The PSK pass (urhgpu_iq_to_bits_batch_psk_dev, below) is this route with k_batch_costas (batch_psk.hip) in k_batch_demod's place.
// Nothing waits for another workgroup; the one atomic is the tie pool's cursor.
#include "batch_kernels.hpp"      // (first: the fp64 forms of URH_FDIV / URH_FSQRT)

#include <algorithm>

#include "msg_state.hpp"

namespace urh {

constexpr int kBdBlock = 256;

// afp_demod (signal_functions.pyx:333-378) of capture c into qad[s0 .. s0 + n): k_batch_bits' rules -- q[0] = noise_val, zeros for n <= 2, a
// refused start or end reads and writes nothing, a noise flag 2 writes two zeros and nothing else.  The predecessor of sample i is sample
// i - 1 of the SAME capture (i >= 1): never the neighbouring capture's sample.
template <int DT, int MOD, bool DNOISE>
__global__ __launch_bounds__(kBdBlock) void k_batch_demod(const RunArgs p, const BatchArgs b) {
    if ((int64_t)blockIdx.x >= b.k) return;
    const int64_t c = b.plan[2 * b.k + blockIdx.x];            // launch order: longest capture first
    if (c < 0 || c >= b.k) return;
    const BatchCapture cap = batch_capture(b, c);              // (n is the samples' alone: a bad plan entry does not stop the demodulation)
    float nsq = 0.0f;
    bool two = false;
    if (DNOISE) {
        const urhgpu_noise_result *r = (const urhgpu_noise_result *)p.d_noise + c;
        nsq = r->noise_sqrd;
        two = r->flag == 2 && cap.n > 2;
    }
    const uint32_t n = two ? 2u : (uint32_t)cap.n;             // < 2^31
    const char *iq = (const char *)b.iq + cap.s0 * Iq<DT>::kBytes;
    float *qad = b.qad + cap.s0;
    if (n <= 2) {                                              // :335-336
        if (threadIdx.x < n) qad[threadIdx.x] = 0.0f;
        return;
    }
    for (uint32_t i = threadIdx.x; i < n; i += kBdBlock) {
        float cc, dd, pc = 0.0f, pd = 0.0f;
        Iq<DT>::load1(iq, i, cc, dd);
        if (MOD == URHGPU_MOD_FSK && i > 0) Iq<DT>::load1(iq, i - 1, pc, pd);
        float q = demod_one<MOD, DT, DNOISE>(pc, pd, cc, dd, p, nsq);
        q = (i == 0) ? p.noise_val : q;                        // :361
        qad[i] = q;
    }
}

// One wavefront per capture behind the chain's k_me_peaks: k_ac_publish's arithmetic -- urhgpu_get_center_thresholds' int -> float conversion,
// fp32 multiply and add / sub (the library is built without contraction) on (float)peak_center where the device has decided (flag 1), on the
// configured center otherwise -- into thr[c][order - 1]; the capture's result block; and for flag 3 alone the histogram's counts into the tie
// pool, reserved by lane 0 with one atomicAdd on the cursor (the trailing block's counts_off).  A capture whose counts do not fit below
// cap_tie gets n_counts = 0: the host then runs the single-range estimator on it.
__global__ __launch_bounds__(64) void k_batch_center_publish(const MsgState *st, const unsigned int *hist, int64_t max_bins, int64_t c0, int kg,
                                                              float cfg_center, float spacing, int order, float *thr,
                                                              urhgpu_batch_center_result *res, int64_t k, unsigned int *tie, int64_t cap_tie) {
    const int m = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (m >= kg) return;
    const int64_t c = c0 + m;
    const MsgState s = st[m];
    const bool decided = s.peak_flag == 1;
    if (thr) {
        const float cen = decided ? (float)s.peak_center : cfg_center;
        const int half = order / 2;
        float *t = thr + c * (int64_t)(order - 1);
        for (int i = lane; i < order - 1; i += 64) t[i] = (i < half) ? cen - (float)(half - (i + 1)) * spacing : cen + (float)(i + 1 - half) * spacing;
    }
    const int64_t nb = s.n_edges >= 2 ? s.n_edges - 1 : 0;
    bool ship = s.peak_flag == 3 && nb > 0 && nb <= max_bins && tie != nullptr;
    int64_t base = 0;
    if (ship) {
        unsigned long long got = 0;
        if (lane == 0) got = atomicAdd((unsigned long long *)&res[k].counts_off, (unsigned long long)nb);
        const uint32_t g_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)got), g_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(got >> 32));
        base = (int64_t)(((uint64_t)g_hi << 32) | g_lo);
        ship = base >= 0 && base <= cap_tie && nb <= cap_tie - base;
    }
    if (lane == 0) {
        urhgpu_batch_center_result r;
        r.r.center = decided ? s.peak_center : 0.0; r.r.flag = s.peak_flag; r.r.n_bins = nb; r.r.e0 = s.e0; r.r.delta = s.delta;
        r.r.kept = s.kept; r.r.trimmed = s.L; r.r.n_counts = ship ? nb : 0;
        r.counts_off = ship ? base : 0;
        res[c] = r;
    }
    if (ship) {
        const unsigned int *y = hist + (int64_t)m * max_bins;  // (k_me_peaks has folded the replicas into the row's first nb counters)
        for (int64_t i = lane; i < nb; i += 64) tie[base + i] = y[i];
    }
}

static int launch_batch_demod(const RunArgs &a, const BatchArgs &b, int dtype, int mod, bool dn, unsigned grid, hipStream_t s) {
    return dispatch_dtype(dtype, [&](auto dt) {
        return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
            return dispatch_bool(dn, [&](auto dnoise) {
                hipLaunchKernelGGL((k_batch_demod<dt.value, m.value, dnoise.value>), dim3(grid), dim3(kBdBlock), 0, s, a, b);
                return URHGPU_OK;
            });
        });
    });
}

// the qad-input walk: MOD x ORDER2 (the sample type plays no part)
static int launch_batch_bits_qin(const RunArgs &a, const BatchArgs &b, int mod, unsigned grid, hipStream_t s) {
    return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
        return dispatch_bool(a.order == 2, [&](auto o2) {
            hipLaunchKernelGGL((k_batch_bits<URHGPU_DT_F32, m.value, o2.value, false, true>), dim3(grid), dim3(64), 0, s, a, b);
            return URHGPU_OK;
        });
    });
}

// the argument checks the center outputs share: capacities against what k captures need
static int center_outputs_check(int64_t k, int order, const void *d_scratch, int64_t scratch_bytes, const BatchCenterScratch &L, const float *d_thr,
                                int64_t cap_thr, const void *d_result, int64_t cap_result, const void *d_tie, int64_t cap_tie) {
    if (scratch_bytes < 0 || cap_thr < 0 || cap_result < 0 || cap_tie < 0) return URHGPU_ERR_ARG;
    if (k > 0 && (!d_scratch || !d_result)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_scratch & 255) || ((uintptr_t)d_thr & 3) || ((uintptr_t)d_result & 7) || ((uintptr_t)d_tie & 3) || (cap_tie > 0 && !d_tie)) return URHGPU_ERR_ARG;
    if (k > 0 && (size_t)scratch_bytes < L.bytes) return URHGPU_ERR_CAPACITY;
    if (d_thr && cap_thr < k * (int64_t)(order - 1)) return URHGPU_ERR_CAPACITY;
    if (d_result && cap_result < k + 1) return URHGPU_ERR_CAPACITY;
    return URHGPU_OK;
}

// the chain and the publish step for all groups: kBatchCenterChainLaunches + 1 launches and one fill per group
static int center_groups(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, int64_t k, const urhgpu_params *p, int64_t max_size,
                         const urhgpu_noise_result *d_noise, const BatchCenterScratch &L, char *scratch, float *d_thr, urhgpu_batch_center_result *d_res,
                         unsigned int *d_tie, int64_t cap_tie) {
    const int64_t max_bins = ctx->tune_center_max_bins;
    hipStream_t s = ctx->stream;
    if (d_res) URH_HIP(hipMemsetAsync(d_res + k, 0, sizeof(urhgpu_batch_center_result), s));      // the trailing block: the tie pool's cursor
    for (int64_t c0 = 0; c0 < k; c0 += L.group) {
        const int64_t kg = std::min<int64_t>(L.group, k - c0);
        MsgState *d_st = nullptr;
        unsigned int *d_hist = nullptr;
        URH_TRY(center_stats_batch_async(d_qad, total, d_start, k, d_noise, c0, kg, max_size, max_bins, L, scratch, s, &d_st, &d_hist));
        hipLaunchKernelGGL(k_batch_center_publish, dim3((unsigned)kg), dim3(64), 0, s, (const MsgState *)d_st, (const unsigned int *)d_hist, max_bins, c0, (int)kg,
                           p->center, p->center_spacing, 1 << p->bits_per_symbol, d_thr, d_res, k, d_tie, cap_tie);
        ctx->batch_launches += kBatchCenterChainLaunches + 1;
    }
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_center_plan(const int64_t *lengths, int64_t k, int64_t total, int64_t max_bins, int64_t *scratch_bytes, int64_t *n_groups, int64_t *group) {
    if (k < 0 || k > INT32_MAX || max_bins < 1 || max_bins > (1 << 20) || (k > 0 && total < 0 && !lengths)) return URHGPU_ERR_ARG;
    int64_t sum = 0;
    if (lengths)
        for (int64_t i = 0; i < k; ++i) {
            if (lengths[i] < 0 || lengths[i] > INT32_MAX) return URHGPU_ERR_ARG;
            sum += lengths[i];
        }
    if (total < 0) total = sum;
    const BatchCenterScratch L = batch_center_scratch(k, total, max_bins);
    if (L.n_tiles > INT32_MAX) return URHGPU_ERR_UNSUPPORTED;
    if (scratch_bytes) *scratch_bytes = (int64_t)L.bytes;
    if (n_groups) *n_groups = L.n_groups;
    if (group) *group = L.group;
    return URHGPU_OK;
}

int urhgpu_batch_center_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, int64_t k, const urhgpu_params *p, int64_t max_size,
                            const urhgpu_noise_result *d_noise, void *d_scratch, int64_t scratch_bytes, float *d_thr, int64_t cap_thr, void *d_result,
                            int64_t cap_result, uint32_t *d_tie, int64_t cap_tie) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0 || (k > 0 && !d_start) || (total > 0 && !d_qad)) return URHGPU_ERR_ARG;
    URH_TRY(batch_check_params(p));
    if (((uintptr_t)d_qad & 3) || ((uintptr_t)d_start & 7) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    const BatchCenterScratch L = batch_center_scratch(k, total, ctx->tune_center_max_bins);
    URH_TRY(center_outputs_check(k, 1 << p->bits_per_symbol, d_scratch, scratch_bytes, L, d_thr, cap_thr, d_result, cap_result, d_tie, cap_tie));
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    return center_groups(ctx, d_qad, total, d_start, k, p, max_size, d_noise, L, (char *)d_scratch, d_thr, (urhgpu_batch_center_result *)d_result, d_tie, cap_tie);
}

// the arguments of the qad-input walk: batch_setup's checks and blocks, with the demodulated buffer where the samples were
static int qad_walk_setup(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k, const urhgpu_params *p,
                          const float *d_thr, const urhgpu_noise_result *d_noise, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir,
                          void *d_blob, int64_t cap_blob, RunArgs &a, BatchArgs &b) {
    if ((total > 0 && !d_qad) || ((uintptr_t)d_qad & 3) || ((uintptr_t)d_thr & 3) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    // (batch_setup vouches for a 16-byte aligned sample buffer; the walk reads floats: it is shown the aligned address below d_qad and never follows it)
    URH_TRY(batch_setup(ctx, (const void *)((uintptr_t)d_qad & ~(uintptr_t)15), total, d_start, d_plan, k, p, nullptr, d_work, work_bytes, d_counts, d_dir,
                        d_blob, cap_blob, a, b));
    b.iq = nullptr;
    b.qad = const_cast<float *>(d_qad);                        // (QIN: read, never written)
    a.d_thr = d_thr;
    a.d_noise = (const float *)d_noise;
    return URHGPU_OK;
}

int urhgpu_qad_to_bits_batch_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                 const urhgpu_params *p, const float *d_thr, int64_t cap_thr, const urhgpu_noise_result *d_noise, void *d_work,
                                 int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob) {
    RunArgs a;
    BatchArgs b;
    URH_TRY(qad_walk_setup(ctx, d_qad, total, d_start, d_plan, k, p, d_thr, d_noise, d_work, work_bytes, d_counts, d_dir, d_blob, cap_blob, a, b));
    if (d_thr && (cap_thr < 0 || cap_thr < k * (int64_t)(a.order - 1))) return URHGPU_ERR_CAPACITY;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    URH_TRY(launch_batch_bits_qin(a, b, p->mod, grid, ctx->stream));
    launch_batch_scan_pack(b, grid, ctx->stream);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_iq_to_bits_batch_center_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                       const urhgpu_params *p, int auto_noise, int64_t max_size, float *d_qad, void *d_work, int64_t work_bytes,
                                       int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob, urhgpu_noise_result *d_noise, void *d_scratch,
                                       int64_t scratch_bytes, float *d_thr, int64_t cap_thr, void *d_result, int64_t cap_result, uint32_t *d_tie,
                                       int64_t cap_tie) {
    if (!d_qad || (auto_noise && k > 0 && !d_noise) || ((uintptr_t)d_noise & 7) || (k > 0 && !d_thr)) return URHGPU_ERR_ARG;
    RunArgs a;
    BatchArgs b;
    URH_TRY(batch_setup(ctx, d_iq, total, d_start, d_plan, k, p, d_qad, d_work, work_bytes, d_counts, d_dir, d_blob, cap_blob, a, b));
    const BatchCenterScratch L = batch_center_scratch(k, total, ctx->tune_center_max_bins);
    URH_TRY(center_outputs_check(k, a.order, d_scratch, scratch_bytes, L, d_thr, cap_thr, d_result, cap_result, d_tie, cap_tie));
    const urhgpu_noise_result *noise = auto_noise ? d_noise : nullptr;
    a.d_noise = (const float *)noise;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    if (auto_noise) {
        URH_TRY(urhgpu_batch_noise_dev(ctx, d_iq, total, d_start, d_plan, k, p, d_noise));       // (counts its launch)
    }
    URH_TRY(launch_batch_demod(a, b, p->dtype, p->mod, auto_noise != 0, grid, ctx->stream));
    ctx->batch_launches += 1;
    URH_TRY(center_groups(ctx, d_qad, total, d_start, k, p, max_size, noise, L, (char *)d_scratch, d_thr, (urhgpu_batch_center_result *)d_result, d_tie, cap_tie));
    a.d_thr = d_thr;
    b.iq = nullptr;
    URH_TRY(launch_batch_bits_qin(a, b, p->mod, grid, ctx->stream));
    launch_batch_scan_pack(b, grid, ctx->stream);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// The whole PSK pass (include/urhgpu.h "a batch of captures: PSK"): urhgpu_iq_to_bits_batch_center_dev with k_batch_costas (batch_psk.hip) where
// that demodulates, and the center chain only when asked for.  Everything behind the demodulation reads qad and the noise value alone, and
// PSK shares -4 with FSK: the argument blocks are batch_setup's for the parameters recoded as FSK, the walk is its FSK instantiation (no
// ASK rule), and the noise launch reads the sample type alone.
int urhgpu_iq_to_bits_batch_psk_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                    const urhgpu_params *p, int auto_noise, int auto_center, int64_t max_size, float *d_qad, void *d_work,
                                    int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob, urhgpu_noise_result *d_noise,
                                    void *d_scratch, int64_t scratch_bytes, float *d_thr, int64_t cap_thr, void *d_result, int64_t cap_result,
                                    uint32_t *d_tie, int64_t cap_tie) {
    if (!d_qad || (auto_noise && k > 0 && !d_noise) || ((uintptr_t)d_noise & 7) || (auto_center && k > 0 && !d_thr)) return URHGPU_ERR_ARG;
    URH_TRY(batch_costas_check(p));
    urhgpu_params q = *p;
    q.mod = URHGPU_MOD_FSK;
    RunArgs a;
    BatchArgs b;
    URH_TRY(batch_setup(ctx, d_iq, total, d_start, d_plan, k, &q, d_qad, d_work, work_bytes, d_counts, d_dir, d_blob, cap_blob, a, b));
    BatchCenterScratch L;
    if (auto_center) {
        L = batch_center_scratch(k, total, ctx->tune_center_max_bins);
        URH_TRY(center_outputs_check(k, a.order, d_scratch, scratch_bytes, L, d_thr, cap_thr, d_result, cap_result, d_tie, cap_tie));
    }
    const urhgpu_noise_result *noise = auto_noise ? d_noise : nullptr;
    a.d_noise = (const float *)noise;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    if (auto_noise) {
        URH_TRY(urhgpu_batch_noise_dev(ctx, d_iq, total, d_start, d_plan, k, &q, d_noise));      // (counts its launch)
    }
    URH_TRY(launch_batch_costas(p, b, noise, ctx->stream));
    ctx->batch_launches += 1;
    if (auto_center) {
        URH_TRY(center_groups(ctx, d_qad, total, d_start, k, &q, max_size, noise, L, (char *)d_scratch, d_thr, (urhgpu_batch_center_result *)d_result, d_tie,
                              cap_tie));
    }
    a.d_thr = auto_center ? d_thr : nullptr;
    b.iq = nullptr;
    URH_TRY(launch_batch_bits_qin(a, b, q.mod, grid, ctx->stream));
    launch_batch_scan_pack(b, grid, ctx->stream);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                           const urhgpu_params *p, const urhgpu_noise_result *d_noise, float *d_qad) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0) return URHGPU_ERR_ARG;
    URH_TRY(batch_check_params(p));
    if (k > 0 && (!d_start || !d_plan)) return URHGPU_ERR_ARG;
    if ((total > 0 && (!d_iq || !d_qad)) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_qad & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    RunArgs a;
    BatchArgs b;
    batch_run_args(p, a);
    memset(&b, 0, sizeof(b));                              // no work buffer: batch_capture then vouches for the samples alone
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total; b.qad = d_qad;
    b.sps = p->samples_per_symbol; b.bps = p->bits_per_symbol; b.tol = p->tolerance;
    a.d_noise = (const float *)d_noise;
    URH_TRY(launch_batch_demod(a, b, p->dtype, p->mod, d_noise != nullptr, (unsigned)std::max<int64_t>(k, 1), ctx->stream));
    ctx->batch_launches += 1;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_center_fetch(urhgpu_ctx *ctx, const void *d_result, int64_t k, const uint32_t *d_tie, int64_t cap_tie, void *h_result, uint32_t *h_tie,
                              int64_t cap_host, int64_t *used) {
    if (!ctx || k < 0 || !d_result || !h_result || cap_tie < 0 || cap_host < 0 || !used) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemcpyAsync(h_result, d_result, (size_t)(k + 1) * sizeof(urhgpu_batch_center_result), hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    const int64_t cursor = ((const urhgpu_batch_center_result *)h_result)[k].counts_off;
    const int64_t n = std::min<int64_t>(cursor, cap_tie);     // (captures behind the pool's end reserved but did not store)
    *used = n;
    if (n < 0) return URHGPU_ERR_ARG;
    if (n == 0) return URHGPU_OK;
    if (n > cap_host) return URHGPU_ERR_CAPACITY;
    if (!d_tie || !h_tie) return URHGPU_ERR_ARG;
    URH_HIP(hipMemcpyAsync(h_tie, d_tie, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
