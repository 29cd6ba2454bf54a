// batch.hip -- many short captures in one pass: a WAVEFRONT PER CAPTURE (include/urhgpu.h "a batch of captures").
//
// A pass over one capture is all fixed cost below a few hundred thousand samples (a dozen launches whose kernels run for
// microseconds).  Here the parallelism is ACROSS captures instead: K captures lie back to back in one buffer, three launches serve
// all of them, and inside a capture the reference's two state machines are followed almost literally by one wavefront:
//   k_batch_bits   afp_demod (signal_functions.pyx:333-378) on kBatchStep consecutive samples per step, one per lane, with the
//                  primitives of the hot kernels (demod_prims.hpp); the step's run boundaries by ballot; grab_pulse_lens
//                  (:392-495) over those runs in wave-uniform code; the rows into the capture's region of the work buffer; then
//                  _ppseq_to_bits (ProtocolAnalyzer.py:323-414) over the stored rows, the lanes expanding a row's symbols
//   k_batch_scan   exclusive prefix of the captures' compact-blob sizes: the directory
//   k_batch_pack   every capture's standard compact blob (compact.hpp) at its directory offset, a wavefront per capture
// Nothing here waits for another wavefront, uses an atomic or touches the hot kernel's data structures.  k_batch_bits and what it is built
// from live in batch_kernels.hpp, which batch_auto.hip instantiates too (every capture gated with its own detected threshold).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "batch_kernels.hpp"

namespace urh {

// dir[i] = bytes of the blobs of the captures before i; dir[k] = all of them.  One workgroup: thread t owns a contiguous stretch.
__global__ __launch_bounds__(256) void k_batch_scan(const BatchArgs b) {
    __shared__ int64_t part[256];
    const int t = (int)threadIdx.x;
    const int64_t per = (b.k + 255) / 256, lo = (t * per < b.k) ? t * per : b.k, hi = (lo + per < b.k) ? lo + per : b.k;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += batch_blob_layout(b.counts + kBatchCounts * i).total;
    part[t] = sum;
    __syncthreads();
    int64_t off = 0;
    for (int j = 0; j < t; ++j) off += part[j];
    for (int64_t i = lo; i < hi; ++i) { b.dir[i] = off; off += batch_blob_layout(b.counts + kBatchCounts * i).total; }
    if (t == 255) b.dir[b.k] = off;
}

static int launch_batch_bits(const RunArgs &a, const BatchArgs &b, int dtype, int mod, unsigned grid, hipStream_t s) {
    return dispatch_dtype(dtype, [&](auto dt) {
        return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
            return dispatch_bool(a.order == 2, [&](auto o2) {
                hipLaunchKernelGGL((k_batch_bits<dt.value, m.value, o2.value>), dim3(grid), dim3(64), 0, s, a, b);
                return URHGPU_OK;
            });
        });
    });
}

// the ranges of the other passes, whatever the modulation
static int batch_check_ranges(const urhgpu_params *p) {
    if (!p) return URHGPU_ERR_ARG;
    if (p->dtype < URHGPU_DT_I8 || p->dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (p->tolerance < 0 || p->tolerance > 65535 || p->samples_per_symbol < 1 || p->bits_per_symbol < 1) return URHGPU_ERR_ARG;
    if (p->bits_per_symbol > 7) return URHGPU_ERR_UNSUPPORTED;
    return URHGPU_OK;
}

// the parameters a batch accepts (every entry point below, and batch_auto.hip's): ASK / FSK, the ranges of the other passes
int batch_check_params(const urhgpu_params *p) {
    URH_TRY(batch_check_ranges(p));
    // (the walk follows a wavefront per capture: PSK has entry points of its own, batch_psk.hip, whose loop is a lane per capture)
    if (p->mod != URHGPU_MOD_ASK && p->mod != URHGPU_MOD_FSK) return URHGPU_ERR_UNSUPPORTED;
    return URHGPU_OK;
}

// ... and what the PSK entry points accept (batch_psk.hip): the same ranges, PSK alone
int batch_check_params_psk(const urhgpu_params *p) {
    URH_TRY(batch_check_ranges(p));
    if (p->mod != URHGPU_MOD_PSK) return URHGPU_ERR_UNSUPPORTED;
    return URHGPU_OK;
}

// the demodulation's argument block from the parameters of a batch (p has passed batch_check_params)
void batch_run_args(const urhgpu_params *p, RunArgs &a) {
    memset(&a, 0, sizeof(a));
    a.order = 1 << p->bits_per_symbol;
    urhgpu_get_center_thresholds(p->center, p->center_spacing, a.order, a.thr);
    a.noise_sqrd = p->noise_threshold * p->noise_threshold;
    a.noise_val = p->mod == URHGPU_MOD_ASK ? 0.0f : -4.0f;                      // get_noise_for_mod_type (:31-44)
    a.tol = p->tolerance;
    switch (p->dtype) {                                                        // :343-354 (double sqrt of the integer constant, stored to float)
        case URHGPU_DT_I8: a.max_magnitude = (float)sqrt(32513.0); break;
        case URHGPU_DT_U8: a.max_magnitude = (float)sqrt(65025.0); break;
        case URHGPU_DT_I16: a.max_magnitude = (float)sqrt(2147418113.0); break;
        case URHGPU_DT_U16: a.max_magnitude = (float)sqrt(4294836225.0); break;
        default: a.max_magnitude = (float)sqrt(2.0); break;
    }
}

// the argument checks of urhgpu_iq_to_bits_batch_dev and the two argument blocks of its launches (shared with batch_auto.hip)
int batch_setup(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k, const urhgpu_params *p,
                float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob, RunArgs &a, BatchArgs &b) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0 || work_bytes < 0 || cap_blob < 0 || !d_dir) return URHGPU_ERR_ARG;
    URH_TRY(batch_check_params(p));
    if (k > 0 && (!d_start || !d_plan || !d_counts)) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || (work_bytes > 0 && !d_work) || (cap_blob > 0 && !d_blob)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_blob & 15) || ((uintptr_t)d_qad & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_dir & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    batch_run_args(p, a);
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total; b.qad = d_qad;
    b.work = (char *)d_work; b.work_bytes = work_bytes; b.counts = d_counts; b.dir = d_dir; b.blob = (char *)d_blob; b.cap_blob = cap_blob;
    b.pause_threshold = p->pause_threshold; b.sps = p->samples_per_symbol; b.bps = p->bits_per_symbol; b.tol = p->tolerance;
    b.each = nullptr; b.each_thr = nullptr; b.n_thr = 0; b.each_lo = 0; b.each_n = 0;      // (one parameter set for all)
    return URHGPU_OK;
}

void launch_batch_scan(const BatchArgs &b, hipStream_t s) { hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(256), 0, s, b); }

void launch_batch_scan_pack(const BatchArgs &b, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(256), 0, s, b);
    hipLaunchKernelGGL(k_batch_pack<false>, dim3(grid), dim3(64), 0, s, b);
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_step(void) { return kBatchStep; }

int urhgpu_batch_plan(const int64_t *lengths, int64_t k, const urhgpu_params *p, int policy, int64_t cap_rows_fixed, int64_t *plan,
                      int64_t *work_bytes, int64_t *blob_capacity) {
    if (k < 0 || (k > 0 && (!lengths || !plan)) || policy < 0 || policy > 2 || (policy == 2 && cap_rows_fixed < 0)) return URHGPU_ERR_ARG;
    URH_TRY(batch_check_params(p));
    const int64_t sps = (int64_t)p->samples_per_symbol;
    int64_t work = 0, blob = 0;
    for (int64_t i = 0; i < k; ++i) {
        const int64_t n = lengths[i];
        if (n < 0 || n > INT32_MAX) return URHGPU_ERR_ARG;
        const int64_t bound = n / ((int64_t)p->tolerance + 1) + 2;             // accepted runs cannot be denser than one per tolerance + 1 samples
        int64_t rows = bound;
        if (policy == 0) rows = std::min<int64_t>(bound, std::max<int64_t>(64, 4 * (n / sps) + 64));
        if (policy == 2) rows = std::min<int64_t>(cap_rows_fixed, INT32_MAX);
        const BatchRegion R = batch_region(n, rows, p->samples_per_symbol, p->bits_per_symbol);
        plan[i] = work;
        plan[k + i] = rows;
        work += R.bytes;
        blob += urh::blob_capacity(R.cap_rows, R.cap_bits, R.cap_msg, 0, 0);
    }
    if (k > 0) {
        std::vector<int64_t> order((size_t)k);
        std::iota(order.begin(), order.end(), int64_t(0));
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return lengths[a] > lengths[b]; });
        std::copy(order.begin(), order.end(), plan + 2 * k);
    }
    if (work_bytes) *work_bytes = work;
    if (blob_capacity) *blob_capacity = blob;
    return URHGPU_OK;
}

int urhgpu_iq_to_bits_batch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                const urhgpu_params *p, float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir,
                                void *d_blob, int64_t cap_blob) {
    RunArgs a;
    BatchArgs b;
    URH_TRY(batch_setup(ctx, d_iq, total, d_start, d_plan, k, p, d_qad, d_work, work_bytes, d_counts, d_dir, d_blob, cap_blob, a, b));
    // three launches whatever k and the lengths are (k = 0: grids of one workgroup that finds nothing to do; the scan writes dir[0] = 0)
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1);
    URH_TRY(launch_batch_bits(a, b, p->dtype, p->mod, grid, ctx->stream));
    launch_batch_scan_pack(b, grid, ctx->stream);
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_fetch(urhgpu_ctx *ctx, const int64_t *d_dir, int64_t k, const void *d_blob, int64_t *h_dir, void *h_blob, int64_t cap_host,
                       int64_t *total_bytes) {
    if (!ctx || !d_dir || k < 0 || !h_dir || cap_host < 0 || !total_bytes) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemcpyAsync(h_dir, d_dir, (size_t)(k + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    const int64_t total = h_dir[k];
    *total_bytes = total;
    if (total < 0) return URHGPU_ERR_ARG;
    if (total > cap_host) return URHGPU_ERR_CAPACITY;
    if (total == 0) return URHGPU_OK;
    if (!d_blob || !h_blob) return URHGPU_ERR_ARG;
    URH_HIP(hipMemcpyAsync(h_blob, d_blob, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

int urhgpu_batch_launches(urhgpu_ctx *ctx, int64_t *out2) {
    if (!ctx || !out2) return URHGPU_ERR_ARG;
    out2[0] = (int64_t)ctx->batch_launches;
    out2[1] = (int64_t)ctx->batch_copies;
    return URHGPU_OK;
}

}  // extern "C"
