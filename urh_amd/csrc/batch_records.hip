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
#include "batch_kernels.hpp"

#include <algorithm>

#include "rec_sum.hpp"

namespace urh {

struct BatchRecArgs {
    BatchArgs b;                 // the walk's block: iq, start (of k_all captures), plan, k, total, work, counts, sps, bps, pause_threshold
    int64_t k_all;               // captures d_start describes (k without a map)
    const int64_t *map;          // nullptr, or [k]: capture j's samples are capture map[j]'s of b.start
    int64_t *rec_dir;            // [k + 1]
    urhgpu_msg_record *rec;
    int32_t *rec_capture;        // [cap_rec] the capture (of b.start) a record's samples lie in
    int64_t cap_rec;
    int64_t divisor;             // <= 1: no padding
    double norm;
};

// the stored messages of capture c as every kernel here counts them: the walk's count, never more than its row capacity allows
__device__ __forceinline__ int64_t rec_msgs(const BatchRecArgs &a, int64_t c) {
    const int64_t n = a.b.counts[kBatchCounts * c + 1], rows = a.b.plan[a.b.k + c];
    const int64_t cap = (rows < 0 || rows > 0x7fffffffll) ? 0 : rows / 2 + 1;
    return n < 0 ? 0 : (n < cap ? n : cap);
}

// capture c's samples and its region as the walk derived them (batch_capture), the samples taken through the map
struct RecCapture { int64_t src, s0, n, roff; BatchRegion R; bool ok; };
__device__ __forceinline__ bool rec_samples(const BatchRecArgs &a, int64_t src, int64_t *s0, int64_t *n) {
    if (src < 0 || src >= a.k_all) return false;
    const int64_t lo = a.b.start[src], hi = a.b.start[src + 1];
    if (!(lo >= 0 && hi >= lo && hi <= a.b.total && hi - lo <= 0x7fffffffll)) return false;
    *s0 = lo; *n = hi - lo;
    return true;
}
__device__ __forceinline__ RecCapture rec_capture_of(const BatchRecArgs &a, int64_t c) {
    RecCapture v;
    v.src = a.map ? a.map[c] : c;
    v.s0 = 0; v.n = 0;
    v.ok = rec_samples(a, v.src, &v.s0, &v.n);
    v.roff = a.b.plan[c];
    const int64_t cap_rows = a.b.plan[a.b.k + c];
    v.R = batch_region(v.n, v.ok ? cap_rows : 0, a.b.sps, a.b.bps);
    if (cap_rows < 0 || cap_rows > 0x7fffffffll || v.roff < 0 || (v.roff & 15) || v.roff > a.b.work_bytes || v.R.bytes > a.b.work_bytes - v.roff) v.ok = false;
    return v;
}

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

__device__ __forceinline__ void rec_store(const BatchRecArgs &a, int64_t at, int64_t first, int64_t mid, int64_t n_pad, int flag, int64_t src) {
    if (at < 0 || at >= a.cap_rec) return;                 // a message beyond the record capacity is not stored
    urhgpu_msg_record r;
    r.rssi = __builtin_nan(""); r.first_pos = first; r.mid_pos = mid; r.n_pad = (int32_t)n_pad; r.flag = flag;
    a.rec[at] = r;
    a.rec_capture[at] = (int32_t)src;
}

__global__ __launch_bounds__(64) void k_batch_rec_pos(const BatchRecArgs a) {
    const int lane = (int)threadIdx.x;
    if ((int64_t)blockIdx.x >= a.b.k) return;
    const int64_t c = a.b.plan[2 * a.b.k + blockIdx.x];        // launch order: longest capture first
    if (c < 0 || c >= a.b.k) return;
    const RecCapture cap = rec_capture_of(a, c);
    const int64_t n_msg = rec_msgs(a, c), base = a.rec_dir[c];
    const int64_t *cnt = a.b.counts + kBatchCounts * c;
    const int64_t nr = cnt[0];
    // a capture whose results were truncated or refused: flag 0 for what it stored; nothing of its region is followed
    const bool sweep = cap.ok && !(cnt[4] & (1 | kBatchBadStart)) && nr >= 0 && nr <= cap.R.cap_rows && n_msg <= cap.R.cap_msg;
    int64_t m = 0;                                             // messages closed so far: the record the sweep writes next
    if (sweep) {
        const char *region = a.b.work + cap.roff;
        const int2 *rows = (const int2 *)(region + cap.R.off_rows);
        const int64_t *msg_off = (const int64_t *)(region + cap.R.off_msg_off), *pauses = (const int64_t *)(region + cap.R.off_pauses);
        const int64_t pt = a.b.pause_threshold, sps = a.b.sps;
        const int64_t spb = (int64_t)(a.b.sps / (uint32_t)a.b.bps);       // int(samples_per_symbol / bits_per_symbol)
        int64_t ts = 0;                                        // total_samples in front of the row
        int64_t nb = 0;                                        // bits gathered for message m
        bool there_was_data = false, have_t = false;
        int64_t first = 0, pos_t = 0;                          // positions of the message's bit 0 and bit t
        // message m as the walk stored it, read before its rows: L bits, n_pad zero bits borrowed, k the middle index after the padding,
        // t = min(k, L - 1) the bit whose position the record needs unless the middle lies at or behind the closing pause's start
        int64_t L = -1, n_pad = 0, k = 0, t = 0;
#define REC_LOAD_MSG() \
        do { \
            L = -1; n_pad = 0; k = 0; t = 0; \
            if (m < n_msg) { \
                L = msg_off[m + 1] - msg_off[m]; \
                n_pad = rec_n_pad(L, pauses[m], sps, a.divisor); \
                k = (L + n_pad) / 2; \
                t = k < L - 1 ? k : L - 1; \
            } \
        } while (0)
        // closed: np = L + 2 entries, entry L = A, the closing pause's start; trailing: np = L + 1.  k_msg_records: in_pad = n_pad > 0 && k > np - 2,
        // rel = in_pad ? np - 2 : k, mid = pos[rel] + (in_pad ? (k - rel) * sps : 0)
#define REC_CLOSE(closed_, A_) \
        do { \
            const bool c_ok = m < n_msg && L >= 1 && nb == L && have_t; \
            int64_t mid = pos_t; \
            if (closed_) { if (k >= L) mid = (A_) + (k - L) * sps; } \
            else if (k > L - 1) mid = pos_t + (k - (L - 1)) * sps; \
            if (lane == 0 && m < n_msg) rec_store(a, base + m, c_ok ? first : 0, c_ok ? mid : 0, n_pad, c_ok ? 1 : 0, cap.src); \
            ++m; \
        } while (0)
        REC_LOAD_MSG();
        for (int64_t rb = 0; rb < nr; rb += 64) {
            int len_v = 0, st_v = 0, nsym_v = 0;
            if (rb + lane < nr) {
                const int2 row = rows[rb + lane];
                len_v = row.x; st_v = row.y;
                // int(L / sps) + (fraction > 0.5), as k_batch_bits takes it
                const uint32_t q = (uint32_t)(len_v < 0 ? -(int64_t)len_v : (int64_t)len_v), qq = q / a.b.sps, rr = q - qq * a.b.sps;
                nsym_v = len_v < 0 ? -(int)qq : (int)(qq + ((2 * (uint64_t)rr > (uint64_t)a.b.sps) ? 1u : 0u));
            }
            const int cnt_rows = (int)((nr - rb < 64) ? (nr - rb) : 64);
            for (int j = 0; j < cnt_rows; ++j) {
                const int64_t len = batch_lane(len_v, j), nsym = batch_lane(nsym_v, j);
                const int s = batch_lane(st_v, j);
                if (rb + j == 0 && s == -1) { ts += len; continue; }           // "starts with pause": only seeds total_samples
                if (s == -1 && !(nsym <= pt || pt == 0)) {                     // a long pause
                    if (there_was_data) {
                        REC_CLOSE(true, ts);
                        REC_LOAD_MSG();
                        there_was_data = false;
                    }
                    nb = 0; have_t = false;                                    // (without data: drops what was gathered)
                    ts += len;
                    continue;
                }
                const int64_t k_bits = nsym * a.b.bps;
                if (k_bits > 0) {
                    if (nb == 0) first = ts;
                    if (!have_t && t >= nb && t < nb + k_bits) { pos_t = ts + (t - nb) * spb; have_t = true; }
                    nb += k_bits;
                }
                if (s != -1 && !there_was_data && nsym > 0) there_was_data = true;
                ts += len;
            }
        }
        if (there_was_data) REC_CLOSE(false, ts);
#undef REC_CLOSE
#undef REC_LOAD_MSG
        if (m > n_msg) m = n_msg;
    }
    // what the sweep did not reach (all of a truncated or refused capture's): flag 0
    for (int64_t i = m + lane; i < n_msg; i += 64) rec_store(a, base + i, 0, 0, 0, 0, cap.src);
}

template <int DT>
__global__ __launch_bounds__(kRecThreads) void k_batch_msg_records(const BatchRecArgs a) {
    __shared__ RecShared sh;
    const int tid = threadIdx.x;
    int64_t n_rec = a.rec_dir[a.b.k];
    if (n_rec > a.cap_rec) n_rec = a.cap_rec;
    for (int64_t i = blockIdx.x; i < n_rec; i += gridDim.x) {
        // ---- the record's window: Python's slice of the capture the message lies in (every thread alike) ----
        const int64_t mid = a.rec[i].mid_pos;
        const bool ok = a.rec[i].flag == 1;
        int64_t s0 = 0, n_c = 0, lo = 0, w = 0;
        const bool there = ok && rec_samples(a, a.rec_capture[i], &s0, &n_c);
        if (there) py_slice(mid, mid + (int64_t)a.b.sps, n_c, &lo, &w);       // lo + w <= n_c: no load leaves [start[c], start[c + 1])
        // ---- np.mean of the window's terms ----
        const double total = rec_window_sum<DT>(sh, a.b.iq, s0 + lo, w, a.norm);
        if (tid == 0) {
            const bool good = there && !sh.bad;
            a.rec[i].rssi = (good && w > 0) ? total / (double)w : __builtin_nan("");
            a.rec[i].flag = good ? 1 : (there ? -1 : 0);
        }
        __syncthreads();                                               // (the next message's round starts from a clean state)
    }
}

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
    hipLaunchKernelGGL(k_batch_rec_pos, dim3(grid), dim3(64), 0, s, a);
    switch (p->dtype) {
        case URHGPU_DT_I8: hipLaunchKernelGGL(k_batch_msg_records<URHGPU_DT_I8>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_U8: hipLaunchKernelGGL(k_batch_msg_records<URHGPU_DT_U8>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_I16: hipLaunchKernelGGL(k_batch_msg_records<URHGPU_DT_I16>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_U16: hipLaunchKernelGGL(k_batch_msg_records<URHGPU_DT_U16>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        default: hipLaunchKernelGGL(k_batch_msg_records<URHGPU_DT_F32>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
    }
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
