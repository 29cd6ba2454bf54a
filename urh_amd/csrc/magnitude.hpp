// magnitude.hpp -- one sample's magnitude (util.pyx:128-136) for every sample type, shared by the kernels that reduce magnitudes
// (filters.hip: get_magnitudes and the chunk statistics of detect_noise_level; shard_estimators.hip: the same statistics of a shard).
// float input -> (double) sqrtf(I*I + Q*Q) in fp32; integer input -> products and sum in C `int` (wrapping, as the reference's
// generated code), sqrt in double.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urhgpu.h"

// the correctly rounded fp32 square root; a translation unit may define its own form first (demod_prims.hpp has the same default)
#ifndef URH_FSQRT
#define URH_FSQRT(x) __builtin_sqrtf(x)
#endif

namespace urh {

template <int DT> struct MagLoad;
template <> struct MagLoad<URHGPU_DT_F32> {
    static __device__ __forceinline__ double mag(const void *p, int64_t i) {
        const float2 v = ((const float2 *)p)[i];
        return (double)URH_FSQRT(v.x * v.x + v.y * v.y);
    }
};
template <class T2> __device__ __forceinline__ double int_mag(int re, int im) {
    const int s = (int)((unsigned)(re * re) + (unsigned)(im * im));
    return __builtin_sqrt((double)s);
}
template <> struct MagLoad<URHGPU_DT_I8> {
    static __device__ __forceinline__ double mag(const void *p, int64_t i) { const char2 v = ((const char2 *)p)[i]; return int_mag<void>(v.x, v.y); }
};
template <> struct MagLoad<URHGPU_DT_U8> {
    static __device__ __forceinline__ double mag(const void *p, int64_t i) { const uchar2 v = ((const uchar2 *)p)[i]; return int_mag<void>(v.x, v.y); }
};
template <> struct MagLoad<URHGPU_DT_I16> {
    static __device__ __forceinline__ double mag(const void *p, int64_t i) { const short2 v = ((const short2 *)p)[i]; return int_mag<void>(v.x, v.y); }
};
template <> struct MagLoad<URHGPU_DT_U16> {
    static __device__ __forceinline__ double mag(const void *p, int64_t i) {
        const ushort2 v = ((const ushort2 *)p)[i];
        // 65535^2 overflows C int: wrap like the reference (unsigned arithmetic, same two's-complement bits)
        const int s = (int)((unsigned)v.x * (unsigned)v.x + (unsigned)v.y * (unsigned)v.y);
        return __builtin_sqrt((double)s);
    }
};

}  // namespace urh
