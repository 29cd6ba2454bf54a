// dc_sub.hpp -- the subtraction of DC correction for one component, every sample type: shared by the correction of one capture
// (dc_correct.hip) and of a batch of captures (batch_dc.hip), so that the two cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace urh {

template <class T, class M> __device__ __forceinline__ T dc_sub(T x, M m) {
    if constexpr (std::is_same<T, float>::value) return x - m;
    else return (T)(int)((double)x - m);             // truncated toward zero into an int32, low bits kept: numpy's cast on x86-64
}

}  // namespace urh
