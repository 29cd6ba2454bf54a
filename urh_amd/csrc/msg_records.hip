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
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "launchers.hpp"
#include "magnitude.hpp"
#include "pairwise.hpp"
#include "pass.hpp"

using namespace urh;

namespace {

constexpr int kRecThreads = 256, kRecLeaves = kRecThreads / 8, kRecOps = 160, kRecStack = 48, kRecMaxBlocks = 1024;

struct RecArgs {
    const void *iq;
    int64_t n;
    const int64_t *msg_off, *pauses, *pos_off, *pos, *counts;
    int64_t cap_msg, cap_pos, cap_rec;
    int64_t sps, divisor;        // divisor <= 1: no padding
    double norm;                 // sqrt(min^2 + max^2) of the sample type
    urhgpu_msg_record *rec;
};

struct RecFrame { int64_t off, len; int stage; };

// Python's a[start:stop] on n elements: where the slice begins and how many elements it has
__device__ __forceinline__ void py_slice(int64_t start, int64_t stop, int64_t n, int64_t *lo, int64_t *count) {
    const int64_t a = start < 0 ? (start + n < 0 ? 0 : start + n) : (start > n ? n : start);
    const int64_t b = stop < 0 ? (stop + n < 0 ? 0 : stop + n) : (stop > n ? n : stop);
    *lo = a;
    *count = b > a ? b - a : 0;
}

template <int DT>
__global__ __launch_bounds__(kRecThreads) void k_msg_records(RecArgs a) {
    __shared__ RecFrame s_frames[kRecStack];
    __shared__ double s_values[kRecStack];
    __shared__ double s_acc[kRecThreads];
    __shared__ double s_leaf_sum[kRecLeaves];
    __shared__ int64_t s_leaf_off[kRecLeaves];
    __shared__ int s_leaf_len[kRecLeaves];
    __shared__ unsigned char s_ops[kRecOps];
    __shared__ int s_sp, s_vsp, s_n_leaves, s_n_ops, s_bad;
    URH_TAIL_PRIO();
    const int tid = threadIdx.x, grp = tid >> 3, j = tid & 7;
    int64_t n_msg = a.counts[1];
    if (n_msg > a.cap_msg) n_msg = a.cap_msg;
    if (n_msg > a.cap_rec) n_msg = a.cap_rec;
    int64_t n_pos = a.counts[3];
    if (n_pos > a.cap_pos) n_pos = a.cap_pos;
    for (int64_t m = blockIdx.x; m < n_msg; m += gridDim.x) {
        // ---- the message's scalars: padding, first and middle position, window (every thread alike) ----
        const int64_t L = a.msg_off[m + 1] - a.msg_off[m], pause = a.pauses[m], po = a.pos_off[m], np = a.pos_off[m + 1] - po;
        int64_t n_pad = 0;
        if (a.divisor > 1 && L >= 0) {
            const int64_t missing = (a.divisor - L % a.divisor) % a.divisor;
            if (missing > 0 && pause >= a.sps * missing) n_pad = missing;
        }
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
        auto term = [&](int64_t i) -> double { return MagLoad<DT>::mag(a.iq, lo + i) / a.norm; };
        // ---- np.mean of the window's terms: piece after piece of 8192, each in rounds of (emit leaves, sum leaves, run the additions) ----
        double total = 0.0;                                            // (thread 0's: ((0 + pw(piece 0)) + pw(piece 1)) + ...)
        if (tid == 0) s_bad = 0;
        __syncthreads();
        for (int64_t piece = 0; piece < w && !s_bad; piece += kPwChunk) {
            __syncthreads();                                               // (every thread has read s_bad)
            if (tid == 0) {
                s_vsp = 0; s_sp = 1;
                s_frames[0].off = piece; s_frames[0].len = w - piece < kPwChunk ? w - piece : kPwChunk; s_frames[0].stage = 0;
            }
            __syncthreads();
            while (s_sp > 0 && !s_bad) {                                   // (shared: every thread reads the same values behind the barrier)
                __syncthreads();                                           // ... and all of them before thread 0 writes them again
                if (tid == 0) {
                    int sp = s_sp, nl = 0, no = 0;
                    while (sp > 0 && nl < kRecLeaves && no < kRecOps) {
                        RecFrame f = s_frames[sp - 1];
                        if (f.len <= kPwLeaf) {
                            s_leaf_off[nl] = f.off; s_leaf_len[nl] = (int)f.len; ++nl;
                            s_ops[no++] = 0; --sp;
                        } else if (f.stage == 2) {
                            s_ops[no++] = 1; --sp;
                        } else if (sp >= kRecStack) {
                            s_bad = 1; break;                              // (deeper than any 64-bit length goes)
                        } else {
                            const int64_t n2 = pw_split(f.len);
                            s_frames[sp - 1].stage = f.stage + 1;
                            s_frames[sp].off = f.stage == 0 ? f.off : f.off + n2;
                            s_frames[sp].len = f.stage == 0 ? n2 : f.len - n2;
                            s_frames[sp].stage = 0;
                            ++sp;
                        }
                    }
                    s_sp = sp; s_n_leaves = nl; s_n_ops = no;
                }
                __syncthreads();
                const int nl = s_n_leaves;
                int len = 0, lim = 0;
                int64_t off = 0;
                if (grp < nl) {
                    len = s_leaf_len[grp]; off = s_leaf_off[grp]; lim = len - (len % 8);
                    if (len >= 8) {
                        double r = term(off + j);
                        for (int i = 8; i < lim; i += 8) r += term(off + i + j);
                        s_acc[tid] = r;
                    }
                }
                __syncthreads();
                if (grp < nl && j == 0) {
                    double res;
                    if (len < 8) {
                        res = 0.0;
                        for (int i = 0; i < len; ++i) res += term(off + i);
                    } else {
                        const double *r = s_acc + tid;
                        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                        for (int i = lim; i < len; ++i) res += term(off + i);
                    }
                    s_leaf_sum[grp] = res;
                }
                __syncthreads();
                if (tid == 0) {
                    int vsp = s_vsp, li = 0;
                    for (int o = 0; o < s_n_ops; ++o) {
                        if (s_ops[o] == 0) {
                            if (vsp < kRecStack) s_values[vsp] = s_leaf_sum[li];
                            else s_bad = 1;
                            ++vsp; ++li;
                        } else {
                            if (vsp >= 2 && vsp <= kRecStack) s_values[vsp - 2] = s_values[vsp - 2] + s_values[vsp - 1];
                            else s_bad = 1;
                            --vsp;
                        }
                    }
                    s_vsp = vsp;
                }
                __syncthreads();
            }
            if (tid == 0) {
                if (s_vsp == 1 && !s_bad) total += s_values[0];
                else s_bad = 1;
            }
            __syncthreads();
        }
        if (tid == 0) {
            urhgpu_msg_record r;
            const bool good = ok && !s_bad;
            r.rssi = (good && w > 0) ? total / (double)w : __builtin_nan("");
            r.first_pos = first; r.mid_pos = mid;
            r.n_pad = (int32_t)n_pad; r.flag = good ? 1 : (ok ? -1 : 0);  // (-1: the summation's bookkeeping gave up -- not reached for any 64-bit length)
            a.rec[m] = r;
        }
        __syncthreads();                                               // (the next message's round starts from a clean state)
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

}  // namespace

namespace urh {

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
    switch (p->dtype) {
        case URHGPU_DT_I8: hipLaunchKernelGGL(k_msg_records<URHGPU_DT_I8>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_U8: hipLaunchKernelGGL(k_msg_records<URHGPU_DT_U8>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_I16: hipLaunchKernelGGL(k_msg_records<URHGPU_DT_I16>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        case URHGPU_DT_U16: hipLaunchKernelGGL(k_msg_records<URHGPU_DT_U16>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
        default: hipLaunchKernelGGL(k_msg_records<URHGPU_DT_F32>, dim3(blocks), dim3(kRecThreads), 0, s, a); break;
    }
    URH_HIP(hipGetLastError());
    if (h_rec) {
        hipLaunchKernelGGL(k_msg_records_mirror, dim3(1), dim3(64), 0, s, (const uint4 *)d_rec, (uint4 *)h_rec, out->counts, out->cap_msg, cap_rec);
        URH_HIP(hipGetLastError());
    }
    return URHGPU_OK;
}

}  // namespace urh

extern "C" {

int urhgpu_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out,
                           int64_t message_length_divisor, void *d_rec, int64_t cap_msg, void *h_rec) {
    if (!ctx) return URHGPU_ERR_ARG;
    RecordsScope scope;                                      // (host waits below here are counted: urhgpu_test_records_host_syncs)
    URH_HIP(hipSetDevice(ctx->device));
    // behind the pass: on the tail stream while a pipelined pass's tail is pending there, on the context's stream otherwise
    const bool on_tail = ctx->pipelined && ctx->tail_pending && ctx->tail_stream && ctx->last_tail == ctx->tail_stream;
    hipStream_t s = on_tail ? ctx->tail_stream : ctx->stream;
    URH_TRY(launch_msg_records(d_iq, n, p, out, message_length_divisor, d_rec, cap_msg, h_rec, s));
    // urhgpu_ctx_join waits for the event of the pass recorded last: move it behind the records
    if (on_tail) URH_HIP(hipEventRecord(ctx->ev_tail[(ctx->flip + 2) % 3], ctx->tail_stream));
    return URHGPU_OK;
}

int64_t urhgpu_test_records_host_syncs(void) { return (int64_t)urh::g_records_host_syncs.load(); }

}  // extern "C"
