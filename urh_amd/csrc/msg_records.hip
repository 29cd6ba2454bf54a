// msg_records.hip -- one record per message behind a pass (include/urhgpu.h "message records inside a pass"): the ASK padding decision,
// the first and the middle bit's position and the RSSI of ProtocolAnalyzer.get_protocol_from_signal (ProtocolAnalyzer.py:256-272), while the
// capture is still in device memory.
//
// k_msg_records: one workgroup of 256 threads per message, a bounded grid that strides over the messages (n_msg is read from the pass's
// counts on the device).  Every thread reads the message's few scalars (uniform loads) and decides the padding and the window; the RSSI
// is the float64 np.mean of the window's normalised magnitudes, summed in numpy's order (pairwise.hpp states it for float32; a contiguous
// float64 np.add.reduce is walked in the same pieces of 8192 elements, total = ((0 + pw(piece 0)) + pw(piece 1)) + ..., with float64
// accumulators -- tests/test_msg_records_host.py holds that against numpy for every length up to 20 000, and a fixture of the real
// reference with a window of 9000 samples pins it).  Per piece:
//     thread 0 walks the pw_split tree depth first and emits up to 32 leaves (at most 128 terms each) and the additions that follow them;
//     eight lanes per leaf build the leaf's eight strided accumulators in parallel (lane j: terms j, 8 + j, ...), the group's first lane
//     combines them in numpy's order and adds the leaf's tail; thread 0 then runs the emitted additions on a value stack.
// A window of a few thousand terms -- samples_per_symbol is tens to a few thousand -- takes one or two rounds (4096 terms are exactly 32
// leaves), a longer one more rounds and pieces of the same code: exact for every length, no second form.  The terms are formed from global memory when they are added (each is used once; the
// eight lanes of a leaf read eight neighbouring samples), not staged.
// k_msg_records_mirror: one wavefront stores the n_msg records into the pinned host mirror, 16 bytes per lane, contiguously.
// The summation is the device function rec_window_sum (rec_sum.hpp: batch_records.hip calls it too), shared with the records of a sharded capture (include/urhgpu.h "message records of a
// sharded capture"): k_shard_msg_records is k_msg_records on one rank's outputs -- global positions, samples read at mid - pos_base -- with the
// first message closed on the rank taken from a descriptor built from gathered data and its window from the shard or from a buffer assembled
// from the ranks' samples; k_shard_rec_summary / k_shard_rec_lookup (one wavefront each) write the words the ranks exchange.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"
#include "magnitude.hpp"
#include "pairwise.hpp"
#include "pass.hpp"
#include "rec_sum.hpp"

using namespace urh;

namespace {

struct RecArgs {
    const void *iq;
    int64_t n;
    const int64_t *msg_off, *pauses, *pos_off, *pos, *counts;
    int64_t cap_msg, cap_pos, cap_rec;
    int64_t sps, divisor;        // divisor <= 1: no padding
    double norm;                 // sqrt(min^2 + max^2) of the sample type
    urhgpu_msg_record *rec;
};

template <int DT>
__global__ __launch_bounds__(kRecThreads) void k_msg_records(RecArgs a) {
    __shared__ RecShared sh;
    URH_TAIL_PRIO();
    const int tid = threadIdx.x;
    int64_t n_msg = a.counts[1];
    if (n_msg > a.cap_msg) n_msg = a.cap_msg;
    if (n_msg > a.cap_rec) n_msg = a.cap_rec;
    int64_t n_pos = a.counts[3];
    if (n_pos > a.cap_pos) n_pos = a.cap_pos;
    for (int64_t m = blockIdx.x; m < n_msg; m += gridDim.x) {
        // ---- the message's scalars: padding, first and middle position, window (every thread alike) ----
        const int64_t L = a.msg_off[m + 1] - a.msg_off[m], pause = a.pauses[m], po = a.pos_off[m], np = a.pos_off[m + 1] - po;
        const int64_t n_pad = rec_n_pad(L, pause, a.sps, a.divisor);
        // a padded message keeps its entries 0 .. np - 2 (np - 2: the start S of the closing pause, or the last bit of a trailing message whose
        // short pause is borrowed from); np - 1 + t becomes A + (t + 1) * sps for t < n_pad, A that entry np - 2
        const int64_t k = (L + n_pad) / 2;
        const bool in_pad = n_pad > 0 && k > np - 2;                   // the middle index lies in the padded part
        const int64_t rel = in_pad ? np - 2 : k;
        const bool ok = L >= 0 && po >= 0 && np >= 1 && rel >= 0 && rel < np && po + np <= n_pos;
        int64_t first = 0, mid = 0, lo = 0, w = 0;
        if (ok) {
            first = a.pos[po];
            mid = a.pos[po + rel] + (in_pad ? (k - rel) * a.sps : 0);
            py_slice(mid, mid + a.sps, a.n, &lo, &w);
        }
        // ---- np.mean of the window's terms ----
        const double total = rec_window_sum<DT>(sh, a.iq, lo, w, a.norm);
        if (tid == 0) {
            urhgpu_msg_record r;
            const bool good = ok && !sh.bad;
            r.rssi = (good && w > 0) ? total / (double)w : __builtin_nan("");
            r.first_pos = first; r.mid_pos = mid;
            r.n_pad = (int32_t)n_pad; r.flag = good ? 1 : (ok ? -1 : 0);  // (-1: the summation's bookkeeping gave up -- not reached for any 64-bit length)
            a.rec[m] = r;
        }
        __syncthreads();                                               // (the next message's round starts from a clean state)
    }
}

// ---- the records of one rank of a sharded capture (include/urhgpu.h, "message records of a sharded capture") ----------------------------
struct ShardRecArgs {
    RecArgs a;                   // iq: the shard; n: the CAPTURE's length (windows are clipped at its end); positions are global
    int64_t pos_base, n_local;   // the shard holds samples [pos_base, pos_base + n_local)
    int64_t cap_rows, cap_bits;
    const void *window;          // the first message's window, assembled from the ranks' samples (window_len samples; may be null)
    int64_t window_len;
    int64_t first[URHGPU_SHARD_REC_FIRST_WORDS];     // the descriptor of the first message closed here, from the gathered words
};

// have the pass's outputs on this rank stayed inside their capacities (ShardResult.check_capacity)
__device__ __forceinline__ bool shard_caps_held(const int64_t *counts, int64_t cap_rows, int64_t cap_msg, int64_t cap_bits, int64_t cap_pos) {
    return counts[4] <= cap_rows && counts[1] <= cap_msg && counts[2] <= cap_bits && counts[3] <= cap_pos;
}

template <int DT>
__global__ __launch_bounds__(kRecThreads) void k_shard_msg_records(ShardRecArgs s) {
    __shared__ RecShared sh;
    URH_TAIL_PRIO();
    const RecArgs &a = s.a;
    const int tid = threadIdx.x;
    int64_t n_msg = a.counts[1];
    if (n_msg > a.cap_msg) n_msg = a.cap_msg;
    if (n_msg > a.cap_rec) n_msg = a.cap_rec;
    int64_t n_pos = a.counts[3];
    if (n_pos > a.cap_pos) n_pos = a.cap_pos;
    const bool held = shard_caps_held(a.counts, s.cap_rows, a.cap_msg, s.cap_bits, a.cap_pos);
    for (int64_t m = blockIdx.x; m < n_msg; m += gridDim.x) {
        int64_t n_pad, first = 0, mid = 0, lo = 0, w = 0;
        bool ok;
        if (m == 0) {
            // the first message closed here may have begun on earlier ranks: everything about it comes from the gathered data
            n_pad = s.first[3];
            ok = held && s.first[0] == 1 && s.first[6] == 1;
            if (ok) { first = s.first[4]; mid = s.first[5]; }
        } else {
            // every later one starts behind a pause row that ends in this shard: k_msg_records' arithmetic on the rank's own outputs
            const int64_t L = a.msg_off[m + 1] - a.msg_off[m], pause = a.pauses[m], po = a.pos_off[m], np = a.pos_off[m + 1] - po;
            n_pad = rec_n_pad(L, pause, a.sps, a.divisor);
            const int64_t k = (L + n_pad) / 2;
            const bool in_pad = n_pad > 0 && k > np - 2;
            const int64_t rel = in_pad ? np - 2 : k;
            ok = held && L >= 0 && po >= 0 && np >= 1 && rel >= 0 && rel < np && po + np <= n_pos;
            if (ok) {
                first = a.pos[po];
                mid = a.pos[po + rel] + (in_pad ? (k - rel) * a.sps : 0);
            }
        }
        if (ok) py_slice(mid, mid + a.sps, a.n, &lo, &w);
        // where the window's samples are: the assembled buffer (first message only), or the shard -- nothing outside it is ever read
        const bool assembled = m == 0 && s.first[7] == 1 && s.window != nullptr && w <= s.window_len;
        const bool outside = ok && w > 0 && !assembled && (lo < s.pos_base || lo + w > s.pos_base + s.n_local);
        if (outside) w = 0;
        const void *src = assembled ? s.window : a.iq;
        const double total = rec_window_sum<DT>(sh, src, assembled ? 0 : lo - s.pos_base, w, a.norm);
        if (tid == 0) {
            urhgpu_msg_record r;
            const bool good = ok && !outside && !sh.bad;
            r.rssi = (good && w > 0) ? total / (double)w : __builtin_nan("");
            r.first_pos = first; r.mid_pos = mid;
            r.n_pad = (int32_t)n_pad; r.flag = good ? 1 : (!ok ? 0 : (outside ? -2 : -1));
            a.rec[m] = r;
        }
        __syncthreads();
    }
}

// one wavefront: the rank's summary words (include/urhgpu.h), lane i stores word i
__global__ __launch_bounds__(64) void k_shard_rec_summary(const int64_t *msg_off, const int64_t *pauses, const int64_t *pos_off, const int64_t *counts,
                                                          int64_t cap_rows, int64_t cap_msg, int64_t cap_bits, int64_t cap_pos, int64_t pos_base,
                                                          int64_t n_local, int64_t *words) {
    URH_TAIL_PRIO();
    const bool held = shard_caps_held(counts, cap_rows, cap_msg, cap_bits, cap_pos);
    const int64_t n_msg = counts[1] < cap_msg ? counts[1] : cap_msg, n_bits = counts[2] < cap_bits ? counts[2] : cap_bits;
    const int64_t n_pos = counts[3] < cap_pos ? counts[3] : cap_pos;
    int64_t v = 0;
    switch (threadIdx.x) {
        case 0: v = pos_base; break;
        case 1: v = n_local; break;
        case 2: v = n_msg; break;
        case 3: v = n_msg > 0 ? msg_off[1] : n_bits; break;            // bits before the first close (all of them when none closes)
        case 4: v = n_msg > 0 ? pos_off[1] : n_pos; break;
        case 5: v = n_msg > 0 ? n_bits - msg_off[n_msg] : 0; break;    // bits behind the last close
        case 6: v = n_msg > 0 ? n_pos - pos_off[n_msg] : 0; break;
        case 7: v = n_msg > 0 ? pauses[0] : 0; break;
        case 8: v = held ? 1 : 0; break;
        case 9: v = n_pos; break;
        default: break;
    }
    if (threadIdx.x < URHGPU_SHARD_REC_SUMMARY_WORDS) words[threadIdx.x] = v;
}

// one wavefront: values[i] = pos[index[i]] where this rank holds the entry asked for (index[i] >= 0), 0 elsewhere
__global__ __launch_bounds__(64) void k_shard_rec_lookup(const int64_t *pos, const int64_t *counts, int64_t cap_pos, const int64_t *index, int64_t n,
                                                         int64_t *values) {
    URH_TAIL_PRIO();
    const int64_t n_pos = counts[3] < cap_pos ? counts[3] : cap_pos;
    for (int64_t i = threadIdx.x; i < n; i += 64) {
        const int64_t at = index[i];
        values[i] = (at >= 0 && at < n_pos) ? pos[at] : 0;
    }
}

// one wavefront, contiguous 16-byte stores: the records' mirror in pinned host memory
__global__ __launch_bounds__(64) void k_msg_records_mirror(const uint4 *d_rec, uint4 *h_rec, const int64_t *counts, int64_t cap_msg, int64_t cap_rec) {
    URH_TAIL_PRIO();
    int64_t n_msg = counts[1];
    if (n_msg > cap_msg) n_msg = cap_msg;
    if (n_msg > cap_rec) n_msg = cap_rec;
    const int64_t n16 = n_msg * (int64_t)(sizeof(urhgpu_msg_record) / 16);
    for (int64_t i = threadIdx.x; i < n16; i += 64) h_rec[i] = d_rec[i];
}

static_assert(sizeof(urhgpu_msg_record) == 32, "urhgpu_msg_record: 32 bytes (include/urhgpu.h)");

}  // namespace

namespace urh {

double records_norm(int dtype) {
    // np.sqrt(maximum ** 2.0 + minimum ** 2.0) of IQArray.min_max_for_dtype (IQArray.py:85-86, :246-250): exact integers, one sqrt
    switch (dtype) {
        case URHGPU_DT_I8: return sqrt(127.0 * 127.0 + 128.0 * 128.0);
        case URHGPU_DT_U8: return sqrt(255.0 * 255.0);
        case URHGPU_DT_I16: return sqrt(32767.0 * 32767.0 + 32768.0 * 32768.0);
        case URHGPU_DT_U16: return sqrt(65535.0 * 65535.0);
        default: return sqrt(2.0);
    }
}

int launch_msg_records(const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out, int64_t divisor, void *d_rec, int64_t cap_rec,
                       void *h_rec, hipStream_t s) {
    if (!d_iq || n <= 0 || !p || !out || !out->msg_off || !out->pauses || !out->pos_off || !out->pos || !out->counts || !d_rec || cap_rec < 0) return URHGPU_ERR_ARG;
    if (divisor < 1 || divisor > (int64_t(1) << 30) || p->samples_per_symbol < 1) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)h_rec & 15)) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    if ((uintptr_t)d_iq & (uintptr_t)(dtype_bytes(p->dtype) - 1)) return URHGPU_ERR_ARG;
    const int64_t cap = std::min<int64_t>(cap_rec, out->cap_msg);
    if (cap == 0) return URHGPU_OK;
    RecArgs a{d_iq, n, out->msg_off, out->pauses, out->pos_off, out->pos, out->counts, out->cap_msg, out->cap_pos, cap_rec,
              (int64_t)p->samples_per_symbol, p->mod == URHGPU_MOD_ASK ? divisor : 1, records_norm(p->dtype), (urhgpu_msg_record *)d_rec};
    const int blocks = (int)std::min<int64_t>(cap, kRecMaxBlocks);
    URH_TRY(dispatch_dtype(p->dtype, [&](auto dt) {        // (the dtype_bytes check above has refused every other code)
        hipLaunchKernelGGL(k_msg_records<dt.value>, dim3(blocks), dim3(kRecThreads), 0, s, a);
        return URHGPU_OK;
    }));
    URH_HIP(hipGetLastError());
    if (h_rec) {
        hipLaunchKernelGGL(k_msg_records_mirror, dim3(1), dim3(64), 0, s, (const uint4 *)d_rec, (uint4 *)h_rec, out->counts, out->cap_msg, cap_rec);
        URH_HIP(hipGetLastError());
    }
    return URHGPU_OK;
}

}  // namespace urh

namespace {

// behind the pass: on the tail stream while a pipelined pass's tail is pending there, on the context's stream otherwise
bool records_on_tail(const urhgpu_ctx *ctx) { return ctx->pipelined && ctx->tail_pending && ctx->tail_stream && ctx->last_tail == ctx->tail_stream; }

// what every sharded records call asks of the pass's outputs on this rank
int shard_rec_check(const urhgpu_outputs *out) {
    if (!out || !out->msg_off || !out->pauses || !out->pos_off || !out->pos || !out->counts) return URHGPU_ERR_ARG;
    if (out->cap_rows < 0 || out->cap_msg < 0 || out->cap_bits < 0 || out->cap_pos < 0) return URHGPU_ERR_ARG;
    return URHGPU_OK;
}

}  // namespace

extern "C" {

int urhgpu_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out,
                           int64_t message_length_divisor, void *d_rec, int64_t cap_msg, void *h_rec) {
    if (!ctx) return URHGPU_ERR_ARG;
    RecordsScope scope;                                      // (host waits below here are counted: urhgpu_test_records_host_syncs)
    URH_HIP(hipSetDevice(ctx->device));
    const bool on_tail = records_on_tail(ctx);
    hipStream_t s = on_tail ? ctx->tail_stream : ctx->stream;
    URH_TRY(launch_msg_records(d_iq, n, p, out, message_length_divisor, d_rec, cap_msg, h_rec, s));
    // urhgpu_ctx_join waits for the event of the pass recorded last: move it behind the records
    if (on_tail) URH_HIP(hipEventRecord(ctx->ev_tail[(ctx->flip + 2) % 3], ctx->tail_stream));
    return URHGPU_OK;
}

int urhgpu_shard_records_summary_dev(urhgpu_ctx *ctx, int64_t n_local, int64_t pos_base, const urhgpu_outputs *out, void *d_words) {
    if (!ctx || !d_words || n_local < 0 || pos_base < 0) return URHGPU_ERR_ARG;
    URH_TRY(shard_rec_check(out));
    if ((uintptr_t)d_words & 7) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = records_on_tail(ctx) ? ctx->tail_stream : ctx->stream;
    hipLaunchKernelGGL(k_shard_rec_summary, dim3(1), dim3(64), 0, s, out->msg_off, out->pauses, out->pos_off, out->counts, out->cap_rows, out->cap_msg,
                       out->cap_bits, out->cap_pos, pos_base, n_local, (int64_t *)d_words);
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_shard_records_lookup_dev(urhgpu_ctx *ctx, const urhgpu_outputs *out, const void *d_index, int64_t n, void *d_values) {
    if (!ctx || n < 0 || (n > 0 && (!d_index || !d_values))) return URHGPU_ERR_ARG;
    URH_TRY(shard_rec_check(out));
    if (((uintptr_t)d_index & 7) || ((uintptr_t)d_values & 7)) return URHGPU_ERR_ARG;
    if (n == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = records_on_tail(ctx) ? ctx->tail_stream : ctx->stream;
    hipLaunchKernelGGL(k_shard_rec_lookup, dim3(1), dim3(64), 0, s, out->pos, out->counts, out->cap_pos, (const int64_t *)d_index, n, (int64_t *)d_values);
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_shard_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, const urhgpu_params *p,
                                 const urhgpu_outputs *out, int64_t message_length_divisor, const int64_t *first, const void *d_window,
                                 int64_t window_len, void *d_rec, int64_t cap_msg, void *h_rec) {
    if (!ctx || !d_iq || !p || !first || !d_rec || cap_msg < 0) return URHGPU_ERR_ARG;
    if (n_local <= 0 || pos_base < 0 || pos_base > n_total - n_local || window_len < 0 || (window_len > 0 && !d_window)) return URHGPU_ERR_ARG;
    URH_TRY(shard_rec_check(out));
    if (message_length_divisor < 1 || message_length_divisor > (int64_t(1) << 30) || p->samples_per_symbol < 1) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_rec & 15) || ((uintptr_t)h_rec & 15)) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    if (((uintptr_t)d_iq | (uintptr_t)d_window) & (uintptr_t)(dtype_bytes(p->dtype) - 1)) return URHGPU_ERR_ARG;
    const int64_t cap = std::min<int64_t>(cap_msg, out->cap_msg);
    if (cap == 0) return URHGPU_OK;
    URH_HIP(hipSetDevice(ctx->device));
    const bool on_tail = records_on_tail(ctx);
    hipStream_t s = on_tail ? ctx->tail_stream : ctx->stream;
    ShardRecArgs a{};
    a.a = RecArgs{d_iq, n_total, out->msg_off, out->pauses, out->pos_off, out->pos, out->counts, out->cap_msg, out->cap_pos, cap_msg,
                  (int64_t)p->samples_per_symbol, p->mod == URHGPU_MOD_ASK ? message_length_divisor : 1, records_norm(p->dtype), (urhgpu_msg_record *)d_rec};
    a.pos_base = pos_base; a.n_local = n_local; a.cap_rows = out->cap_rows; a.cap_bits = out->cap_bits;
    a.window = window_len > 0 ? d_window : nullptr; a.window_len = window_len;
    for (int i = 0; i < URHGPU_SHARD_REC_FIRST_WORDS; ++i) a.first[i] = first[i];
    const int blocks = (int)std::min<int64_t>(cap, kRecMaxBlocks);
    URH_TRY(dispatch_dtype(p->dtype, [&](auto dt) {        // (the dtype_bytes check above has refused every other code)
        hipLaunchKernelGGL(k_shard_msg_records<dt.value>, dim3(blocks), dim3(kRecThreads), 0, s, a);
        return URHGPU_OK;
    }));
    URH_HIP(hipGetLastError());
    if (h_rec) {
        hipLaunchKernelGGL(k_msg_records_mirror, dim3(1), dim3(64), 0, s, (const uint4 *)d_rec, (uint4 *)h_rec, out->counts, out->cap_msg, cap_msg);
        URH_HIP(hipGetLastError());
    }
    if (on_tail) URH_HIP(hipEventRecord(ctx->ev_tail[(ctx->flip + 2) % 3], ctx->tail_stream));
    return URHGPU_OK;
}

int64_t urhgpu_test_records_host_syncs(void) { return (int64_t)urh::g_records_host_syncs.load(); }

}  // extern "C"
