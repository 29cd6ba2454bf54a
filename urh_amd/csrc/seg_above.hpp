// seg_above.hpp -- is a sample above the noise, as segment_messages_from_magnitudes compares it (auto_interpretation.pyx:55-111 on
// util.get_magnitudes' values).  One definition for the translation units that segment captures: msg_ranges.hip (a capture alone: the trailing
// below-run of k_seg_finish) and batch_estimate.hip (a batch of captures: every sample of k_batch_segments).  The text below is what
// msg_ranges.hip held until the batch needed it too.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "launchers.hpp"

namespace urh {

// magnitude of sample i compared with the threshold as segment_messages_from_magnitudes does (double magnitude > float threshold)
template <int DT> __device__ bool seg_above(const void *iq, int64_t i, float thr);
template <> __device__ bool seg_above<URHGPU_DT_F32>(const void *iq, int64_t i, float thr) {
    const float2 v = ((const float2 *)iq)[i];
    return (double)__builtin_sqrtf(v.x * v.x + v.y * v.y) > (double)thr;
}
__device__ __forceinline__ bool seg_above_int(int re, int im, float thr) {
    const int s = (int)((unsigned)(re * re) + (unsigned)(im * im));
    return __builtin_sqrt((double)s) > (double)thr;
}
template <> __device__ bool seg_above<URHGPU_DT_I8>(const void *iq, int64_t i, float thr) { const char2 v = ((const char2 *)iq)[i]; return seg_above_int(v.x, v.y, thr); }
template <> __device__ bool seg_above<URHGPU_DT_U8>(const void *iq, int64_t i, float thr) { const uchar2 v = ((const uchar2 *)iq)[i]; return seg_above_int(v.x, v.y, thr); }
template <> __device__ bool seg_above<URHGPU_DT_I16>(const void *iq, int64_t i, float thr) { const short2 v = ((const short2 *)iq)[i]; return seg_above_int(v.x, v.y, thr); }
template <> __device__ bool seg_above<URHGPU_DT_U16>(const void *iq, int64_t i, float thr) {
    const ushort2 v = ((const ushort2 *)iq)[i];
    const int s = (int)((unsigned)v.x * (unsigned)v.x + (unsigned)v.y * (unsigned)v.y);
    return __builtin_sqrt((double)s) > (double)thr;
}

template <> __device__ bool seg_above<kDtAboveFlags>(const void *iq, int64_t i, float) { return ((const float *)iq)[i] > 0.5f; }

}  // namespace urh
