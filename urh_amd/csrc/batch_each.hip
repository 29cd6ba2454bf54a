// batch_each.hip -- a batch of captures, EVERY CAPTURE WITH ITS OWN PARAMETERS (include/urhgpu.h "a batch of captures: parameters per
// capture").  A recording session's transmitters are not alike: estimate_batch learns modulation, samples per symbol, center, tolerance and
// noise per capture, and here capture c is demodulated, sliced and turned into bits with table[c], a urhgpu_batch_each record in device
// memory beside its order - 1 slicing thresholds in one shared float table.  The launch count depends neither on the number of captures nor
// on the number of different parameter sets:
//   k_batch_noise (batch_auto.hip)   only with auto_noise: a threshold per capture; without it the host has written the K result blocks
//   k_batch_bits<DT, MOD, .., EACH>  batch_kernels.hpp's walk with its EACH flag:              the wavefront of capture c loads ITS record, its
//                                    thresholds and its noise block through uniform addresses and reads no other capture's.  Modulation
//                                    stays a template parameter: the plan's launch order holds the ASK captures first (longest first),
//                                    then the FSK captures (longest first), and each modulation present gets ONE launch over its slice --
//                                    at most two.  Captures of every order share a launch: the general classification (for order 2 it
//                                    IS the order-2 form: q <= t[0] ? 1 : 2, a NaN and +inf above, -inf and a value on the threshold below)
//   k_batch_scan (batch.hip)         the directory
//   k_batch_pack<EACH>               batch_kernels.hpp's pack: every region laid out from the capture's own samples per symbol and bits per symbol
// No atomics, nothing waits for another wavefront, no load outside [start[c], start[c + 1]), no store outside the capture's region.
#include "batch_records_kernels.hpp"      // (batch_kernels.hpp first: the fp64 forms of URH_FDIV / URH_FSQRT)

#include <algorithm>
#include <numeric>
#include <vector>

namespace urh {

// one walk launch over the launch-order slice [lo, lo + n) of modulation `mod`
static int launch_each_walk(int dtype, int mod, float noise_threshold, const urhgpu_noise_result *d_noise, BatchArgs b, int64_t lo, int64_t n, hipStream_t s) {
    urhgpu_params pp;
    memset(&pp, 0, sizeof(pp));
    pp.dtype = dtype; pp.mod = mod; pp.bits_per_symbol = 1; pp.samples_per_symbol = 1; pp.noise_threshold = noise_threshold; pp.center_spacing = 1.0f;
    RunArgs a;
    batch_run_args(&pp, a);                                // noise_val of the modulation, max_magnitude of the sample type
    a.d_noise = (const float *)d_noise;
    b.each_lo = lo; b.each_n = n;
    const unsigned grid = (unsigned)n;
    return dispatch_dtype(dtype, [&](auto dt) {
        return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
            hipLaunchKernelGGL((k_batch_bits<dt.value, m.value, false, true, false, true>), dim3(grid), dim3(64), 0, s, a, b);
            return URHGPU_OK;
        });
    });
}

// a record of the table as the host accepts it (the device checks every record again: batch_each_ok)
static int each_check(const urhgpu_batch_each &e) {
    if (e.mod != URHGPU_MOD_ASK && e.mod != URHGPU_MOD_FSK) return URHGPU_ERR_UNSUPPORTED;
    if (e.tolerance < 0 || e.tolerance > 65535 || e.samples_per_symbol < 1 || e.bits_per_symbol < 1 || e.thr_first < 0) return URHGPU_ERR_ARG;
    if (e.bits_per_symbol > 7) return URHGPU_ERR_UNSUPPORTED;
    return URHGPU_OK;
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_plan_each(const int64_t *lengths, int64_t k, const urhgpu_batch_each *each, int policy, int64_t cap_rows_fixed, int64_t *plan,
                           int64_t *work_bytes, int64_t *blob_capacity) {
    if (k < 0 || (k > 0 && (!lengths || !plan || !each)) || policy < 0 || policy > 2 || (policy == 2 && cap_rows_fixed < 0)) return URHGPU_ERR_ARG;
    for (int64_t i = 0; i < k; ++i) URH_TRY(each_check(each[i]));
    int64_t work = 0, blob = 0;
    for (int64_t i = 0; i < k; ++i) {
        const int64_t n = lengths[i], sps = (int64_t)each[i].samples_per_symbol;
        if (n < 0 || n > INT32_MAX) return URHGPU_ERR_ARG;
        const int64_t bound = n / ((int64_t)each[i].tolerance + 1) + 2;          // accepted runs cannot be denser than one per tolerance + 1 samples
        int64_t rows = bound;
        if (policy == 0) rows = std::min<int64_t>(bound, std::max<int64_t>(64, 4 * (n / sps) + 64));
        if (policy == 2) rows = std::min<int64_t>(cap_rows_fixed, INT32_MAX);
        const BatchRegion R = batch_region(n, rows, each[i].samples_per_symbol, each[i].bits_per_symbol);
        plan[i] = work;
        plan[k + i] = rows;
        work += R.bytes;
        blob += urh::blob_capacity(R.cap_rows, R.cap_bits, R.cap_msg, 0, 0);
    }
    if (k > 0) {
        // the launch order: the ASK captures, then the FSK captures, each group longest first -- a walk launch takes one group's slice
        std::vector<int64_t> order((size_t)k);
        std::iota(order.begin(), order.end(), int64_t(0));
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            if (each[a].mod != each[b].mod) return each[a].mod < each[b].mod;
            return lengths[a] > lengths[b];
        });
        std::copy(order.begin(), order.end(), plan + 2 * k);
    }
    if (work_bytes) *work_bytes = work;
    if (blob_capacity) *blob_capacity = blob;
    return URHGPU_OK;
}

int urhgpu_iq_to_bits_batch_each_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                     const urhgpu_batch_each *d_each, const float *d_thr, int64_t n_thr, int64_t n_ask, int auto_noise, float *d_qad,
                                     void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob,
                                     urhgpu_noise_result *d_noise) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0 || work_bytes < 0 || cap_blob < 0 || !d_dir || n_thr < 0 || n_ask < 0 || n_ask > k) return URHGPU_ERR_ARG;
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (k > 0 && (!d_start || !d_plan || !d_counts || !d_each || !d_noise || !d_thr)) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || (work_bytes > 0 && !d_work) || (cap_blob > 0 && !d_blob)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_blob & 15) || ((uintptr_t)d_each & 15) || ((uintptr_t)d_qad & 3) ||
        ((uintptr_t)d_thr & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_dir & 7) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    BatchArgs b;
    memset(&b, 0, sizeof(b));
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total; b.qad = d_qad;
    b.work = (char *)d_work; b.work_bytes = work_bytes; b.counts = d_counts; b.dir = d_dir; b.blob = (char *)d_blob; b.cap_blob = cap_blob;
    b.sps = 1; b.bps = 1;                                  // (read by nothing here but k_batch_noise's batch_capture, which takes the samples alone)
    b.each = d_each; b.each_thr = d_thr; b.n_thr = n_thr;
    if (auto_noise) {                                      // one launch, counted there
        urhgpu_params pn;
        memset(&pn, 0, sizeof(pn));
        pn.dtype = dtype; pn.mod = URHGPU_MOD_FSK; pn.bits_per_symbol = 1; pn.samples_per_symbol = 1; pn.center_spacing = 1.0f;
        URH_TRY(urhgpu_batch_noise_dev(ctx, d_iq, total, d_start, d_plan, k, &pn, d_noise));
    }
    // at most two walk launches whatever k, the lengths and the parameter sets are; scan and pack (k = 0: the scan writes dir[0] = 0)
    hipStream_t s = ctx->stream;
    if (n_ask > 0) { URH_TRY(launch_each_walk(dtype, URHGPU_MOD_ASK, 0.0f, d_noise, b, 0, n_ask, s)); ctx->batch_launches += 1; }
    if (k - n_ask > 0) { URH_TRY(launch_each_walk(dtype, URHGPU_MOD_FSK, 0.0f, d_noise, b, n_ask, k - n_ask, s)); ctx->batch_launches += 1; }
    launch_batch_scan(b, s);
    hipLaunchKernelGGL(k_batch_pack<true>, dim3((unsigned)std::max<int64_t>(k, 1)), dim3(64), 0, s, b);
    ctx->batch_launches += 2;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_msg_records_each_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                      const urhgpu_batch_each *d_each, int64_t message_length_divisor, const void *d_work, int64_t work_bytes,
                                      const int64_t *d_counts, int64_t *d_rec_dir, void *d_rec, int64_t cap_rec, int32_t *d_rec_capture) {
    // what needs no device first: these answers are the same without a GPU
    if (dtype < URHGPU_DT_I8 || dtype > URHGPU_DT_F32) return URHGPU_ERR_DTYPE;
    if (message_length_divisor < 1 || message_length_divisor > (int64_t(1) << 30) || cap_rec < 0) return URHGPU_ERR_ARG;
    if (k < 0 || k > INT32_MAX || total < 0 || work_bytes < 0) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_each & 15) || ((uintptr_t)d_rec_capture & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_rec_dir & 7)) return URHGPU_ERR_ARG;
    if (!ctx || !d_rec_dir || (k > 0 && (!d_plan || !d_counts || !d_start || !d_each))) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || (work_bytes > 0 && !d_work) || (cap_rec > 0 && (!d_rec || !d_rec_capture))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    BatchRecArgs a;
    memset(&a, 0, sizeof(a));
    a.b.iq = d_iq; a.b.start = d_start; a.b.plan = d_plan; a.b.k = k; a.b.total = total;
    a.b.work = (char *)const_cast<void *>(d_work); a.b.work_bytes = work_bytes; a.b.counts = const_cast<int64_t *>(d_counts);
    a.b.sps = 1; a.b.bps = 1;
    a.b.each = d_each; a.b.n_thr = INT64_MAX;              // (the thresholds are not read here: a record is judged by its other values)
    a.k_all = k; a.map = nullptr; a.rec_dir = d_rec_dir; a.rec = (urhgpu_msg_record *)d_rec; a.rec_capture = d_rec_capture; a.cap_rec = cap_rec;
    a.divisor = message_length_divisor;                    // (applied per capture, where its record is ASK)
    a.norm = records_norm(dtype);
    // three launches whatever k, the lengths, the parameter sets and the number of messages are
    hipStream_t s = ctx->stream;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1), blocks = (unsigned)std::max<int64_t>(std::min<int64_t>(cap_rec, kRecMaxBlocks), 1);
    launch_batch_rec_dir(a, s);
    hipLaunchKernelGGL(k_batch_rec_pos<true>, dim3(grid), dim3(64), 0, s, a);
    URH_TRY(dispatch_dtype(dtype, [&](auto dt) {           // (the range check above has refused every other code)
        hipLaunchKernelGGL((k_batch_msg_records<dt.value, true>), dim3(blocks), dim3(kRecThreads), 0, s, a);
        return URHGPU_OK;
    }));
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // extern "C"
