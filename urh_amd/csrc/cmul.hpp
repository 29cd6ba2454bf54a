// complex64 product exactly as GCC emits it for std::complex<float> / float _Complex (shared by the FIR and Costas kernels), and its
// complex128 sibling (the IIR kernels)
#pragma once
#include <hip/hip_runtime.h>

namespace urh {

// ---- complex64 product exactly as GCC emits it for std::complex<float> / float _Complex --------------------
__device__ __forceinline__ float2 mulsc3_recover_inline(float a, float b, float c, float d, float2 r) {
    // libgcc __mulsc3 (C99 G.5.1): only reached when both parts are NaN
    const float ac = a * c, bd = b * d, ad = a * d, bc = b * c;
    bool recalc = false;
    if (isinf(a) || isinf(b)) {
        a = copysignf(isinf(a) ? 1.f : 0.f, a); b = copysignf(isinf(b) ? 1.f : 0.f, b);
        if (isnan(c)) c = copysignf(0.f, c);
        if (isnan(d)) d = copysignf(0.f, d);
        recalc = true;
    }
    if (isinf(c) || isinf(d)) {
        c = copysignf(isinf(c) ? 1.f : 0.f, c); d = copysignf(isinf(d) ? 1.f : 0.f, d);
        if (isnan(a)) a = copysignf(0.f, a);
        if (isnan(b)) b = copysignf(0.f, b);
        recalc = true;
    }
    if (!recalc && (isinf(ac) || isinf(bd) || isinf(ad) || isinf(bc))) {
        if (isnan(a)) a = copysignf(0.f, a);
        if (isnan(b)) b = copysignf(0.f, b);
        if (isnan(c)) c = copysignf(0.f, c);
        if (isnan(d)) d = copysignf(0.f, d);
        recalc = true;
    }
    if (recalc) {
        r.x = __builtin_inff() * (a * c - b * d);
        r.y = __builtin_inff() * (a * d + b * c);
    }
    return r;
}
__device__ __noinline__ inline float2 mulsc3_recover(float a, float b, float c, float d, float2 r) { return mulsc3_recover_inline(a, b, c, d, r); }
__device__ __forceinline__ float2 cmul(float2 x, float2 h) {
    float2 r;
    r.x = x.x * h.x - x.y * h.y;
    r.y = x.x * h.y + x.y * h.x;
    if (__builtin_expect((r.x != r.x) & (r.y != r.y), 0)) r = mulsc3_recover(x.x, x.y, h.x, h.y, r);
    return r;
}

// ---- complex128 product as GCC emits it for std::complex<double> / double _Complex (the IIR's coefficient * sample) ----
__device__ __noinline__ inline double2 muldc3_recover(double a, double b, double c, double d, double2 r) {
    // libgcc __muldc3 (C99 G.5.1): only reached when both parts are NaN
    const double ac = a * c, bd = b * d, ad = a * d, bc = b * c;
    bool recalc = false;
    if (isinf(a) || isinf(b)) {
        a = copysign(isinf(a) ? 1.0 : 0.0, a); b = copysign(isinf(b) ? 1.0 : 0.0, b);
        if (isnan(c)) c = copysign(0.0, c);
        if (isnan(d)) d = copysign(0.0, d);
        recalc = true;
    }
    if (isinf(c) || isinf(d)) {
        c = copysign(isinf(c) ? 1.0 : 0.0, c); d = copysign(isinf(d) ? 1.0 : 0.0, d);
        if (isnan(a)) a = copysign(0.0, a);
        if (isnan(b)) b = copysign(0.0, b);
        recalc = true;
    }
    if (!recalc && (isinf(ac) || isinf(bd) || isinf(ad) || isinf(bc))) {
        if (isnan(a)) a = copysign(0.0, a);
        if (isnan(b)) b = copysign(0.0, b);
        if (isnan(c)) c = copysign(0.0, c);
        if (isnan(d)) d = copysign(0.0, d);
        recalc = true;
    }
    if (recalc) {
        r.x = __builtin_inf() * (a * c - b * d);
        r.y = __builtin_inf() * (a * d + b * c);
    }
    return r;
}
__device__ __forceinline__ double2 cmul128(double2 x, double2 h) {
    double2 r;
    r.x = x.x * h.x - x.y * h.y;
    r.y = x.x * h.y + x.y * h.x;
    if (__builtin_expect((r.x != r.x) & (r.y != r.y), 0)) r = muldc3_recover(x.x, x.y, h.x, h.y, r);
    return r;
}

}  // namespace urh
