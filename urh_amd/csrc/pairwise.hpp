// numpy's float32 summation order (np.add.reduce over a contiguous array), shared by every kernel that has to reproduce it
// (estimators.hip: np.mean / np.var of detect_center; chunk_stats.hip: np.mean(chunk ** 2.0) of the live sniffer's noise gate).
//
// np.add.reduce walks the array in pieces of the ufunc buffer size (8192 elements) and accumulates
//     total = (((0 + pw(piece 0)) + pw(piece 1)) + ...)
// where pw is the pairwise routine of numpy/core/src/umath/loops_utils.h.src (float32 accumulators):
//   n < 8            : res = 0; res += a[i] in order
//   n <= 128         : 8 accumulators r[j] = a[j]; r[j] += a[i + j] for i = 8, 16, ... < n - n % 8;
//                      res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the n % 8 tail in order
//   n > 128          : n2 = n / 2; n2 -= n2 % 8; pw(a, n2) + pw(a + n2, n - n2)
// A full piece is therefore a perfect binary tree over 64 leaves of 128 elements.
//
// float64 (np.mean of a contiguous float64 array: the RSSI of msg_records.hip): the SAME order with float64 accumulators -- the array is
// walked in pieces of kPwChunk elements too, total = ((0 + pw(piece 0)) + pw(piece 1)) + ..., and pw splits by pw_split down to leaves of at
// most kPwLeaf terms; a leaf's eight accumulators may be built by eight lanes and are combined by pw_combine8 below.  Held against numpy for every length from 1 to 20 000 (tests/test_msg_records_host.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace urh {

constexpr int kPwChunk = 8192, kPwLeaf = 128, kPwLeavesPerChunk = kPwChunk / kPwLeaf;

// where pw splits a block of n > kPwLeaf elements: the left part's length
__host__ __device__ inline int64_t pw_split(int64_t n) {
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return n2;
}

// pw over one leaf (n <= kPwLeaf); elem(i) is element i of the leaf
template <typename F>
__device__ __forceinline__ float pw_leaf(int n, F elem) {
    float res;
    if (n < 8) {
        res = 0.f;
        for (int i = 0; i < n; ++i) res += elem(i);
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = elem(j);
        int i;
        for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += elem(i + j);
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += elem(i);
    }
    return res;
}

// the eight accumulators of a leaf of 8 .. kPwLeaf terms, combined in numpy's order (float64 form: the accumulators built lane-parallel)
__device__ __forceinline__ double pw_combine8(const double *r) {
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

}  // namespace urh
