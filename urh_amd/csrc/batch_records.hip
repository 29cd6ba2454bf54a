// batch_records.hip -- one record per message of a BATCH of captures (include/urhgpu.h "a batch of captures: message records per capture"):
// what msg_records.hip queues behind a pass, queued behind the walk of a batch (batch.hip, batch_auto.hip, batch_center.hip), three launches
// whatever the number of captures, their lengths and the number of messages:
//   k_batch_rec_dir        one workgroup: the exclusive prefix of the captures' stored messages, rec_dir[c] = where capture c's records begin,
//                          rec_dir[k] = M, the messages of the whole batch (k_batch_scan's shape)
//   k_batch_rec_pos        a WAVEFRONT PER CAPTURE, in the plan's launch order: a batch ships no positions -- they are a function of the
//                          pulse table --, so the three entries a record needs are derived from the capture's stored {length, state} rows,
//                          64 rows per load, with the control flow of the second half of k_batch_bits (the leading pause only seeds
//                          total_samples; a long pause closes a message or drops what was gathered; the trailing message) and the arithmetic
//                          of host_bits.positions_from_rows: a bit's position is total_samples + j * int(sps / bps) inside its row, entry L of
//                          a closed message is the start of its closing pause.  The message's length and pause are read from the walk's
//                          msg_off / pauses BEFORE its rows are swept, so the middle index is known and ONE sweep suffices.  Lane 0 stores
//                          first_pos, mid_pos, n_pad and a provisional flag into rec[rec_dir[c] + m], and the capture the samples lie in
//                          into rec_capture[] beside it
//   k_batch_msg_records    k_msg_records' second half: a workgroup of 256 threads per message, a bounded grid that strides over the M
//                          messages (M is read on the device); the window is Python's slice of THE CAPTURE -- [mid, mid + sps) clipped at
//                          start[c + 1] - start[c], not at the buffer's end: the next capture lies directly behind --, summed by
//                          rec_window_sum (rec_sum.hpp: the one copy of numpy's float64 order).  No load leaves [start[c], start[c + 1]).
// Nothing here waits for another wavefront or uses an atomic.  batch_kernels.hpp comes first (its rule); the fp32 square root of a float32
// magnitude is then taken in fp64 and rounded once, which is the correctly rounded fp32 root k_msg_records takes.
#include "batch_records_kernels.hpp"

#include <algorithm>

namespace urh {

// rec_dir[i] = records of the captures before i; rec_dir[k] = all of them.  One workgroup: thread t owns a contiguous stretch.
__global__ __launch_bounds__(256) void k_batch_rec_dir(const BatchRecArgs a) {
    __shared__ int64_t part[256];
    const int t = (int)threadIdx.x;
    const int64_t k = a.b.k, per = (k + 255) / 256, lo = (t * per < k) ? t * per : k, hi = (lo + per < k) ? lo + per : k;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += rec_msgs(a, i);
    part[t] = sum;
    __syncthreads();
    int64_t off = 0;
    for (int j = 0; j < t; ++j) off += part[j];
    for (int64_t i = lo; i < hi; ++i) { a.rec_dir[i] = off; off += rec_msgs(a, i); }
    if (t == 255) a.rec_dir[k] = off;
}

void launch_batch_rec_dir(const BatchRecArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_batch_rec_dir, dim3(1), dim3(256), 0, s, a); }

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, int64_t k_all, const int64_t *d_map,
                                 const int64_t *d_plan, int64_t k, const urhgpu_params *p, const urhgpu_noise_result *d_noise,
                                 int64_t message_length_divisor, const void *d_work, int64_t work_bytes, const int64_t *d_counts, int64_t *d_rec_dir,
                                 void *d_rec, int64_t cap_rec, int32_t *d_rec_capture) {
    // what needs no device first: these answers are the same without a GPU
    URH_TRY(batch_check_params(p));
    if (message_length_divisor < 1 || message_length_divisor > (int64_t(1) << 30) || cap_rec < 0) return URHGPU_ERR_ARG;
    if (k < 0 || k > INT32_MAX || k_all < 0 || k_all > INT32_MAX || total < 0 || work_bytes < 0 || (!d_map && k_all != k)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_rec_capture & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_map & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_counts & 7) || ((uintptr_t)d_rec_dir & 7) ||
        ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    if (!ctx || !d_rec_dir || (k > 0 && (!d_plan || !d_counts)) || (k_all > 0 && !d_start)) return URHGPU_ERR_ARG;
    if ((total > 0 && !d_iq) || (work_bytes > 0 && !d_work) || (cap_rec > 0 && (!d_rec || !d_rec_capture))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    BatchRecArgs a;
    memset(&a, 0, sizeof(a));
    a.b.iq = d_iq; a.b.start = d_start; a.b.plan = d_plan; a.b.k = k; a.b.total = total;
    a.b.work = (char *)const_cast<void *>(d_work); a.b.work_bytes = work_bytes; a.b.counts = const_cast<int64_t *>(d_counts);
    a.b.pause_threshold = p->pause_threshold; a.b.sps = p->samples_per_symbol; a.b.bps = p->bits_per_symbol; a.b.tol = p->tolerance;
    a.k_all = k_all; a.map = d_map; a.rec_dir = d_rec_dir; a.rec = (urhgpu_msg_record *)d_rec; a.rec_capture = d_rec_capture; a.cap_rec = cap_rec;
    a.divisor = p->mod == URHGPU_MOD_ASK ? message_length_divisor : 1;
    a.norm = records_norm(p->dtype);
    // three launches whatever k, the lengths and the number of messages are (k = 0: grids of one workgroup that finds nothing to do)
    hipStream_t s = ctx->stream;
    const unsigned grid = (unsigned)std::max<int64_t>(k, 1), blocks = (unsigned)std::max<int64_t>(std::min<int64_t>(cap_rec, kRecMaxBlocks), 1);
    hipLaunchKernelGGL(k_batch_rec_dir, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_batch_rec_pos<false>, dim3(grid), dim3(64), 0, s, a);
    URH_TRY(dispatch_dtype(p->dtype, [&](auto dt) {        // (batch_check_params has refused every other code)
        hipLaunchKernelGGL(k_batch_msg_records<dt.value>, dim3(blocks), dim3(kRecThreads), 0, s, a);
        return URHGPU_OK;
    }));
    ctx->batch_launches += 3;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_batch_records_fetch(urhgpu_ctx *ctx, const void *d_rec, int64_t n_rec, int64_t cap_rec, void *h_rec) {
    if (!ctx || n_rec < 0 || cap_rec < 0 || ((uintptr_t)d_rec & 15) || ((uintptr_t)h_rec & 15)) return URHGPU_ERR_ARG;
    if (n_rec > cap_rec) return URHGPU_ERR_CAPACITY;
    if (n_rec == 0) return URHGPU_OK;
    if (!d_rec || !h_rec) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemcpyAsync(h_rec, d_rec, (size_t)n_rec * sizeof(urhgpu_msg_record), hipMemcpyDeviceToHost, ctx->stream));
    ++ctx->batch_copies;
    URH_HIP(wait_stream(ctx, ctx->stream));
    return URHGPU_OK;
}

}  // extern "C"
