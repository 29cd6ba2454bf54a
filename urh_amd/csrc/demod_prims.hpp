// demod_prims.hpp -- the per-sample primitives of the demodulation: how a sample of each capture type is loaded (Iq<DT>), the reference's
// complex product and atan2f, demod_one (afp_demod's value of one sample) and classify (its state).  Shared by the hot kernels
// (demod_runs.hip) and the batch kernels (batch.hip): one definition, so that both give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmul.hpp"
#include "fdlibm_atan2f.h"
#include "launchers.hpp"
#include "runs.hpp"

namespace urh {

#ifndef URH_NT
#define URH_NT 1          // non-temporal IQ loads / qad stores (streamed once): +8 % on the copy ceiling, tools/kbench
#endif

// the correctly rounded fp32 square root; like URH_FDIV (fdlibm_atan2f.h) a translation unit may define its own form first
#ifndef URH_FSQRT
#define URH_FSQRT(x) __builtin_sqrtf(x)
#endif

template <int DT> struct Iq;
template <> struct Iq<URHGPU_DT_F32> {
    static constexpr int kBytes = 8;
    static __device__ __forceinline__ void load2(const void *b, int64_t i, float &c0, float &d0, float &c1, float &d1) {
#if URH_NT
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f v = __builtin_nontemporal_load((const v4f *)b + (i >> 1)); c0 = v.x; d0 = v.y; c1 = v.z; d1 = v.w;
#else
        float4 v = ((const float4 *)b)[i >> 1]; c0 = v.x; d0 = v.y; c1 = v.z; d1 = v.w;
#endif
    }
    static __device__ __forceinline__ void load1(const void *b, int64_t i, float &c, float &d) {
        float2 v = ((const float2 *)b)[i]; c = v.x; d = v.y;
    }
    // a lane's two samples at `ptr` (16-byte aligned)
    static __device__ __forceinline__ void ld(const void *ptr, float &c0, float &d0, float &c1, float &d1) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f v = __builtin_nontemporal_load((const v4f *)ptr); c0 = v.x; d0 = v.y; c1 = v.z; d1 = v.w;
    }
};
template <> struct Iq<URHGPU_DT_I8> {
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ void load2(const void *b, int64_t i, float &c0, float &d0, float &c1, float &d1) {
        char4 v = ((const char4 *)b)[i >> 1]; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
    static __device__ __forceinline__ void load1(const void *b, int64_t i, float &c, float &d) {
        char2 v = ((const char2 *)b)[i]; c = (float)v.x; d = (float)v.y;
    }
    static __device__ __forceinline__ void ld(const void *ptr, float &c0, float &d0, float &c1, float &d1) {
        char4 v = *(const char4 *)ptr; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
};
template <> struct Iq<URHGPU_DT_U8> {
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ void load2(const void *b, int64_t i, float &c0, float &d0, float &c1, float &d1) {
        uchar4 v = ((const uchar4 *)b)[i >> 1]; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
    static __device__ __forceinline__ void load1(const void *b, int64_t i, float &c, float &d) {
        uchar2 v = ((const uchar2 *)b)[i]; c = (float)v.x; d = (float)v.y;
    }
    static __device__ __forceinline__ void ld(const void *ptr, float &c0, float &d0, float &c1, float &d1) {
        uchar4 v = *(const uchar4 *)ptr; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
};
template <> struct Iq<URHGPU_DT_I16> {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ void load2(const void *b, int64_t i, float &c0, float &d0, float &c1, float &d1) {
        short4 v = ((const short4 *)b)[i >> 1]; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
    static __device__ __forceinline__ void load1(const void *b, int64_t i, float &c, float &d) {
        short2 v = ((const short2 *)b)[i]; c = (float)v.x; d = (float)v.y;
    }
    static __device__ __forceinline__ void ld(const void *ptr, float &c0, float &d0, float &c1, float &d1) {
        short4 v = *(const short4 *)ptr; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
};
template <> struct Iq<URHGPU_DT_U16> {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ void load2(const void *b, int64_t i, float &c0, float &d0, float &c1, float &d1) {
        ushort4 v = ((const ushort4 *)b)[i >> 1]; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
    static __device__ __forceinline__ void load1(const void *b, int64_t i, float &c, float &d) {
        ushort2 v = ((const ushort2 *)b)[i]; c = (float)v.x; d = (float)v.y;
    }
    static __device__ __forceinline__ void ld(const void *ptr, float &c0, float &d0, float &c1, float &d1) {
        ushort4 v = *(const ushort4 *)ptr; c0 = (float)v.x; d0 = (float)v.y; c1 = (float)v.z; d1 = (float)v.w;
    }
};

// conj(a+jb) * (c+jd) exactly as the reference's generated C++ evaluates
//   (s[i-1,0] - imag_unit*s[i-1,1]) * (real + imag_unit*imag)           signal_functions.pyx:375
// with std::complex<float> operands: imag_unit*x is a full complex product (0*x - 1*0, 0*0 + 1*x),
// so signed zeros come out as on the CPU.  For finite non-zero inputs this is
// re = fl(fl(ac)+fl(bd)), im = fl(fl(ad)-fl(bc)).
__device__ __forceinline__ void conj_mul(float a, float b, float c, float d, float &re, float &im) {
    float A = a - 0.0f * b;          // a - (0*b - 1*0)
    float B = 0.0f - (0.0f + b);     // 0 - (0*0 + 1*b)
    float C = c + 0.0f * d;          // c + (0*d - 1*0)
    float D = 0.0f + d;              // 0 + (0*0 + 1*d)
    re = A * C - B * D;
    im = A * D + B * C;
}
// ... with libgcc's recovery where both parts of the product come out NaN (__mulsc3, C99 G.5.1), as the reference's generated C++ has it:
// the general forms (demod_one, fsk_row_general).  An infinite imaginary part makes A or C a NaN (0 * inf); the reference then recovers
// infinite parts and its atan2f gives +-pi/4 or +-3pi/4, not NaN.  (The sites that settle exact zeros keep conj_mul: their products are
// finite.)  Inlined: the hot kernel stays without a call.
__device__ __forceinline__ void conj_mul_general(float a, float b, float c, float d, float &re, float &im) {
    const float A = a - 0.0f * b, B = 0.0f - (0.0f + b), C = c + 0.0f * d, D = 0.0f + d;
    re = A * C - B * D;
    im = A * D + B * C;
    if (__builtin_expect((re != re) & (im != im), 0)) {
        const float2 r = mulsc3_recover_inline(A, B, C, D, make_float2(re, im));
        re = r.x; im = r.y;
    }
}

// Message segmentation (seg_mode) on integer captures: util.get_magnitudes computes I*I + Q*Q in C `int` (wrapping) and
// takes the DOUBLE square root (util.pyx:128-136), and segment_messages_from_magnitudes compares that double with the
// float threshold (auto_interpretation.pyx:82).  The classification only needs "above" / "not above": return a value on
// the right side of every threshold.  (c, d) hold the integer sample exactly (|value| < 2^16).
__device__ __forceinline__ float seg_value_int(float c, float d, float threshold) {
    const int re = (int)c, im = (int)d;
    const int s = (int)((unsigned)(re * re) + (unsigned)(im * im));
    const double m = __builtin_sqrt((double)s);
    return (m > (double)threshold) ? 3.0e38f : -3.0e38f;
}

// atan2f for the common case (both operands finite, non-zero, exponents within 2^60 of each
// other); everything else goes through the literal port in fdlibm_atan2f.h.
__device__ __forceinline__ float atan2f_dev(float y, float x) {
    const uint32_t hx = __float_as_uint(x), hy = __float_as_uint(y);
    const uint32_t ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    const int k = ((int)iy - (int)ix) >> 23;
    const bool special = (ix - 1u >= 0x7f7fffffu) | (iy - 1u >= 0x7f7fffffu) | (k > 60) | (k < -60);
    if (__builtin_expect(special, 0)) return urh_atan2f(y, x);
    const float pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const float r = __uint_as_float(__float_as_uint(URH_FDIV(y, x)) & 0x7fffffffu);
    const uint32_t ir = __float_as_uint(r);
    float z;
    if (ir < 0x3ee00000u) {                       // |y/x| < 0.4375: no argument reduction
        z = (ir < 0x31000000u) ? r : r - urh_atanf_poly(r);
    } else if (ir >= 0x4c000000u) {               // >= 2^25
        z = 1.5707962513e+00f + 7.5497894159e-08f;
    } else {
        float hi, lo, num, den;
        if (ir < 0x3f300000u) { hi = 4.6364760399e-01f; lo = 5.0121582440e-09f; num = 2.0f * r - 1.0f; den = 2.0f + r; }
        else if (ir < 0x3f980000u) { hi = 7.8539812565e-01f; lo = 3.7748947079e-08f; num = r - 1.0f; den = r + 1.0f; }
        else if (ir < 0x401c0000u) { hi = 9.8279368877e-01f; lo = 3.4473217170e-08f; num = r - 1.5f; den = 1.0f + 1.5f * r; }
        else { hi = 1.5707962513e+00f; lo = 7.5497894159e-08f; num = -1.0f; den = r; }
        const float t = URH_FDIV(num, den);
        z = hi - ((urh_atanf_poly(t) - lo) - t);
    }
    const uint32_t m = (hy >> 31) | ((hx >> 30) & 2u);
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

// the state of a sample that is not NOISE from order - 1 thresholds in device memory at t: the ONE text of the device-threshold form, for
// classify<.., true> (t = RunArgs::d_thr) and for a batch's walk, whose captures each have thresholds of their own (batch_kernels.hpp)
template <bool ORDER2>
__device__ __forceinline__ uint32_t classify_thr(float q, const float *t, int order) {
    if (ORDER2) return (q <= t[0]) ? 1u : 2u;
    int st = order - 1;
    for (int k = 0; k < order - 1; ++k)
        if (q <= t[k]) { st = k; break; }
    return (uint32_t)st + 1u;
}

// DTHR (the qad-input instantiations): the thresholds may live in device memory (RunArgs::d_thr) -- plain loads of a uniform address
template <bool ORDER2, bool DTHR = false>
__device__ __forceinline__ uint32_t classify(float q, const RunArgs &p, bool check_noise = true) {
    if (check_noise && q == p.noise_val) return kStPause;
    if (DTHR && p.d_thr) return classify_thr<ORDER2>(q, p.d_thr, p.order);
    if (ORDER2) return (q <= p.thr[0]) ? 1u : 2u;
    int st = p.order - 1;
    for (int k = 0; k < p.order - 1; ++k)
        if (q <= p.thr[k]) { st = k; break; }
    return (uint32_t)st + 1u;
}

// Demodulate one sample.  (pc,pd) = previous IQ sample, (c,d) = this one.
// DN (here and in the helpers of demod_runs.hip): noise_sqrd is the value `nsq` the kernel loaded from device memory (RunArgs::d_noise), not the
// launch argument p.noise_sqrd -- which the instantiations without DN read exactly where they always did
template <int MOD, int DT = URHGPU_DT_F32, bool DN = false>
__device__ __forceinline__ float demod_one(float pc, float pd, float c, float d, const RunArgs &p, float nsq) {
    if (MOD == URHGPU_MOD_ASK && DT != URHGPU_DT_F32 && p.seg_mode) return seg_value_int(c, d, p.thr[0]);
    const float mag = c * c + d * d;
    if (mag <= (DN ? nsq : p.noise_sqrd)) return p.noise_val;
    if (MOD == URHGPU_MOD_ASK) return URH_FDIV(URH_FSQRT(mag), p.max_magnitude);   // (double)sqrtf/(double) == fp32 div
    if (MOD == URHGPU_MOD_FSK) {
        float re, im;
        conj_mul_general(pc, pd, c, d, re, im);
        return atan2f_dev(im, re);
    }
    return 0.0f;   // MOD_OTHER: np.zeros stays
}

}  // namespace urh
