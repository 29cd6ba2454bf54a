// rec_sum.hpp -- the summation of a message record's RSSI window (include/urhgpu.h "message records inside a pass"), shared by the
// translation units that write records: msg_records.hip (a pass, a rank of a sharded capture) and batch_records.hip (a batch of captures).
// The ONE copy of numpy's float64 np.add.reduce order -- pieces of 8192 terms one after the other, each piece pairwise (pairwise.hpp) --
// with what a records kernel decides around it: Python's slice and the ASK padding.  msg_records.hip's head says how a workgroup walks it.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "magnitude.hpp"
#include "pairwise.hpp"

namespace urh {

constexpr int kRecThreads = 256, kRecLeaves = kRecThreads / 8, kRecOps = 160, kRecStack = 48, kRecMaxBlocks = 1024;

struct RecFrame { int64_t off, len; int stage; };

// what one workgroup's summation keeps in LDS (one instance per kernel)
struct RecShared {
    RecFrame frames[kRecStack];
    double values[kRecStack];
    double acc[kRecThreads];
    double leaf_sum[kRecLeaves];
    int64_t leaf_off[kRecLeaves];
    int leaf_len[kRecLeaves];
    unsigned char ops[kRecOps];
    int sp, vsp, n_leaves, n_ops, bad;
};

// Python's a[start:stop] on n elements: where the slice begins and how many elements it has
__device__ __forceinline__ void py_slice(int64_t start, int64_t stop, int64_t n, int64_t *lo, int64_t *count) {
    const int64_t a = start < 0 ? (start + n < 0 ? 0 : start + n) : (start > n ? n : start);
    const int64_t b = stop < 0 ? (stop + n < 0 ? 0 : stop + n) : (stop > n ? n : stop);
    *lo = a;
    *count = b > a ? b - a : 0;
}

// The float64 np.add.reduce of the w terms mag(iq[lo + i]) / norm (the file's head has the order): the ONE copy of the summation, called by
// every thread of the workgroup of both records kernels.  Returns the total to thread 0 (other threads: 0); sh.bad is set where the
// bookkeeping gave up.  Ends behind a barrier.
template <int DT>
__device__ __forceinline__ double rec_window_sum(RecShared &sh, const void *iq, int64_t lo, int64_t w, double norm) {
    const int tid = threadIdx.x, grp = tid >> 3, j = tid & 7;
    auto term = [&](int64_t i) -> double { return MagLoad<DT>::mag(iq, lo + i) / norm; };
    // ---- piece after piece of 8192, each in rounds of (emit leaves, sum leaves, run the additions) ----
    double total = 0.0;                                            // (thread 0's: ((0 + pw(piece 0)) + pw(piece 1)) + ...)
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    for (int64_t piece = 0; piece < w && !sh.bad; piece += kPwChunk) {
        __syncthreads();                                               // (every thread has read sh.bad)
        if (tid == 0) {
            sh.vsp = 0; sh.sp = 1;
            sh.frames[0].off = piece; sh.frames[0].len = w - piece < kPwChunk ? w - piece : kPwChunk; sh.frames[0].stage = 0;
        }
        __syncthreads();
        while (sh.sp > 0 && !sh.bad) {                                 // (shared: every thread reads the same values behind the barrier)
            __syncthreads();                                           // ... and all of them before thread 0 writes them again
            if (tid == 0) {
                int sp = sh.sp, nl = 0, no = 0;
                while (sp > 0 && nl < kRecLeaves && no < kRecOps) {
                    RecFrame f = sh.frames[sp - 1];
                    if (f.len <= kPwLeaf) {
                        sh.leaf_off[nl] = f.off; sh.leaf_len[nl] = (int)f.len; ++nl;
                        sh.ops[no++] = 0; --sp;
                    } else if (f.stage == 2) {
                        sh.ops[no++] = 1; --sp;
                    } else if (sp >= kRecStack) {
                        sh.bad = 1; break;                             // (deeper than any 64-bit length goes)
                    } else {
                        const int64_t n2 = pw_split(f.len);
                        sh.frames[sp - 1].stage = f.stage + 1;
                        sh.frames[sp].off = f.stage == 0 ? f.off : f.off + n2;
                        sh.frames[sp].len = f.stage == 0 ? n2 : f.len - n2;
                        sh.frames[sp].stage = 0;
                        ++sp;
                    }
                }
                sh.sp = sp; sh.n_leaves = nl; sh.n_ops = no;
            }
            __syncthreads();
            const int nl = sh.n_leaves;
            int len = 0, lim = 0;
            int64_t off = 0;
            if (grp < nl) {
                len = sh.leaf_len[grp]; off = sh.leaf_off[grp]; lim = len - (len % 8);
                if (len >= 8) {
                    double r = term(off + j);
                    for (int i = 8; i < lim; i += 8) r += term(off + i + j);
                    sh.acc[tid] = r;
                }
            }
            __syncthreads();
            if (grp < nl && j == 0) {
                double res;
                if (len < 8) {
                    res = 0.0;
                    for (int i = 0; i < len; ++i) res += term(off + i);
                } else {
                    const double *r = sh.acc + tid;
                    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                    for (int i = lim; i < len; ++i) res += term(off + i);
                }
                sh.leaf_sum[grp] = res;
            }
            __syncthreads();
            if (tid == 0) {
                int vsp = sh.vsp, li = 0;
                for (int o = 0; o < sh.n_ops; ++o) {
                    if (sh.ops[o] == 0) {
                        if (vsp < kRecStack) sh.values[vsp] = sh.leaf_sum[li];
                        else sh.bad = 1;
                        ++vsp; ++li;
                    } else {
                        if (vsp >= 2 && vsp <= kRecStack) sh.values[vsp - 2] = sh.values[vsp - 2] + sh.values[vsp - 1];
                        else sh.bad = 1;
                        --vsp;
                    }
                }
                sh.vsp = vsp;
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (sh.vsp == 1 && !sh.bad) total += sh.values[0];
            else sh.bad = 1;
        }
        __syncthreads();
    }
    return total;
}

// the ASK padding of a message of L bits followed by `pause` samples (divisor <= 1: none)
__device__ __forceinline__ int64_t rec_n_pad(int64_t L, int64_t pause, int64_t sps, int64_t divisor) {
    if (divisor > 1 && L >= 0) {
        const int64_t missing = (divisor - L % divisor) % divisor;
        if (missing > 0 && pause >= sps * missing) return missing;
    }
    return 0;
}

// sqrt(min^2 + max^2) of the sample type: what a record's magnitudes are divided by (msg_records.hip)
double records_norm(int dtype);

}  // namespace urh
