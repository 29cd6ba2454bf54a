// costas_prims.hpp -- one step of the Costas loop (costa_demod, signal_functions.pyx:252-330) and the loop's constants, shared by the
// translation units that run the loop: costas.hip (one capture: serial, speculative, sharded) and batch_psk.hip (a batch of captures: a lane
// per capture).  One definition of CostasArgs, CostasState, CostasLoad, the gate, the two forms of the step and costas_args, so that the
// routes cannot drift apart; the text is costas.hip's, moved here unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <math.h>

#include "cmul.hpp"
#include "common.hpp"
#include "glibc_sincosf.h"

namespace urh {

struct CostasArgs {
    const void *iq; int64_t n; float *out;
    float noise_sqrd, alpha, beta, scale, shift;
    int loop_order;
    int warm;                // un-gated samples a candidate runs before its chunk (from the loop bandwidth, see launch_costas)
    // not nullptr: the pass's noise threshold was decided on the device (k_noise_decide) -- every kernel loads noise_sqrd from this device float
    // at its entry (costas_device_noise) instead of taking the launch argument above
    const float *d_noise = nullptr;
};
struct CostasState { float freq, phase; };

__device__ __forceinline__ float costas_clamp(float x) {      // :246-250 (NaN passes through: both comparisons are false)
    float r = (x > 1.0f) ? 1.0f : x;
    r = (x < -1.0f) ? -1.0f : r;
    return r;
}

template <int DT> struct CostasLoad;
template <> struct CostasLoad<URHGPU_DT_F32> { static __device__ __forceinline__ float2 at(const void *p, int64_t i) { return ((const float2 *)p)[i]; } };
template <> struct CostasLoad<URHGPU_DT_I8> { static __device__ __forceinline__ float2 at(const void *p, int64_t i) { const char2 v = ((const char2 *)p)[i]; return make_float2((float)v.x, (float)v.y); } };
template <> struct CostasLoad<URHGPU_DT_U8> { static __device__ __forceinline__ float2 at(const void *p, int64_t i) { const uchar2 v = ((const uchar2 *)p)[i]; return make_float2((float)v.x, (float)v.y); } };
template <> struct CostasLoad<URHGPU_DT_I16> { static __device__ __forceinline__ float2 at(const void *p, int64_t i) { const short2 v = ((const short2 *)p)[i]; return make_float2((float)v.x, (float)v.y); } };
template <> struct CostasLoad<URHGPU_DT_U16> { static __device__ __forceinline__ float2 at(const void *p, int64_t i) { const ushort2 v = ((const ushort2 *)p)[i]; return make_float2((float)v.x, (float)v.y); } };

__device__ __forceinline__ bool costas_gated(float2 sm, const CostasArgs &a) { return sm.x * sm.x + sm.y * sm.y <= a.noise_sqrd; }

// One sample of the loop (:291-328): returns the output, updates the state.  err is only carried for loop orders
// other than 2 / 4 (where it never changes); callers keep it.
// UNIT: float32 captures (shift 0, scale 1): (x + 0.0f) / 1.0f == x + 0.0f for every x, the two IEEE divisions are dropped.
// ORDER: 2 / 4 = the loop order as a compile-time constant (the speculative kernels: five wave-uniform branches less per step);
// 0 = read a.loop_order.
template <bool UNIT = false, int ORDER = 0>
__device__ __forceinline__ float costas_step(float2 sm, CostasState &st, float &err, const CostasArgs &a) {
    const int loop_order = ORDER ? ORDER : a.loop_order;
    if (costas_gated(sm, a)) return -4.0f;                              // NOISE_FSK_PSK, state frozen (:293-295)
    const double two_pi = 2 * 3.14159265358979323846;
    const float real_float = UNIT ? sm.x + 0.0f : (sm.x + a.shift) / a.scale, imag_float = UNIT ? sm.y + 0.0f : (sm.y + a.shift) / a.scale;
    const float2 cur = make_float2(real_float + 0.0f * imag_float, 1.0f * imag_float);   // re + imag_unit * im
    float sn, cs;
    if (urh_sc_abstop12(st.phase) < 0x42f) urh_sincosf_fast(-st.phase, &sn, &cs);        // |phase| < 120: always (the loop keeps it within +-2 pi)
    else { sn = urh_sinf(-st.phase); cs = urh_cosf(-st.phase); }
    const float2 nco = make_float2(cs + 0.0f * sn, 1.0f * sn);
    const float2 z = cmul(nco, cur);
    if (loop_order == 2) {
        err = z.y * z.x;
    } else if (loop_order == 4) {
        const float f1 = z.x > 0.0f ? 1.0f : -1.0f, f2 = z.y > 0.0f ? 1.0f : -1.0f;
        err = f1 * z.y - f2 * z.x;
    }
    err = costas_clamp(err);
    st.freq += a.beta * err;
    st.phase += st.freq + a.alpha * err;
    while ((double)st.phase > two_pi) st.phase = (float)((double)st.phase - two_pi);     // double compare / subtract (:318-321)
    while ((double)st.phase < -two_pi) st.phase = (float)((double)st.phase + two_pi);
    st.freq = costas_clamp(st.freq);
    if (loop_order == 2) return z.x;
    if (loop_order == 4) return (float)(2.0 * (double)z.x + (double)z.y);
    return 0.0f;
}

// The same step as straight-line code (the speculative kernels; loop order 2 or 4): the gate, the two wraps and the clamps are
// selects; what cannot happen in a healthy loop (|phase| beyond 2 pi on entry, a product with two NaN parts) is collected in ONE flag,
// tested once at the end, and sends the whole wavefront through costas_step from the saved state.  Measured effect: small (candidate
// pass 1.97 -> 1.91 ms): nearly every one of a step's ~94 instructions depends on the one before it, a dependent VALU operation
// issues every ~9.5 cycles whatever its type (tools/kbench/lbench.hip: fp32, fp64, conversions alike), and two trajectories per SIMD
// lane cannot fill the gaps -- the pass sits at 94 x 9.5 cycles x 4096 steps.  One wrap is enough when
// |phase| <= 2 pi on entry: |freq'| <= 1 + beta, |alpha err| <= alpha, alpha + beta < 4 for every bandwidth, so |phase'| < 2 pi + 5 < 4 pi.
template <bool UNIT, int ORDER>
__device__ __forceinline__ float costas_step_bf(float2 sm, CostasState &st, float &err, const CostasArgs &a) {
    static_assert(ORDER == 2 || ORDER == 4, "the serial kernel handles the other orders");
    const double two_pi = 2 * 3.14159265358979323846;
    const CostasState old = st;
    const float old_err = err;
    const bool gated = costas_gated(sm, a);
    const float real_float = UNIT ? sm.x + 0.0f : (sm.x + a.shift) / a.scale, imag_float = UNIT ? sm.y + 0.0f : (sm.y + a.shift) / a.scale;
    const float2 cur = make_float2(real_float + 0.0f * imag_float, 1.0f * imag_float);   // re + imag_unit * im
    const bool in_range = __builtin_fabsf(old.phase) <= __uint_as_float(0x40C90FDBu);   // the float next above 2 pi (NaN: false)
    float sn, cs;
    urh_sincosf_fast(-old.phase, &sn, &cs);
    const float2 nco = make_float2(cs + 0.0f * sn, 1.0f * sn);
    float2 z;
    z.x = nco.x * cur.x - nco.y * cur.y;                     // cmul() without its NaN-recovery branch
    z.y = nco.x * cur.y + nco.y * cur.x;
    const bool rare = !gated && (!in_range || ((z.x != z.x) & (z.y != z.y)));
    float e;
    if (ORDER == 2) e = z.y * z.x;
    else {
        const float f1 = z.x > 0.0f ? 1.0f : -1.0f, f2 = z.y > 0.0f ? 1.0f : -1.0f;
        e = f1 * z.y - f2 * z.x;
    }
    e = costas_clamp(e);
    float freq = old.freq + a.beta * e;
    float phase = old.phase + (freq + a.alpha * e);
    const double d = (double)phase;
    const float wrapped_down = (float)(d - two_pi), wrapped_up = (float)(d + two_pi);
    phase = (d > two_pi) ? wrapped_down : ((d < -two_pi) ? wrapped_up : phase);
    freq = costas_clamp(freq);
    const float out = (ORDER == 2) ? z.x : (float)(2.0 * (double)z.x + (double)z.y);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0, 0)) {      // wavefront-uniform; never in a healthy loop
        st = old; err = old_err;
        return costas_step<UNIT, ORDER>(sm, st, err, a);
    }
    st.freq = gated ? old.freq : freq;
    st.phase = gated ? old.phase : phase;
    err = gated ? old_err : e;
    return gated ? -4.0f : out;
}

// Warm-up: two trajectories in the same lock class contract by about (1 - alpha) per sample once the seeded frequency is close;
// from a phase error of order 1 down to the last float bit takes ~ 18 / alpha samples (130 at the default bandwidth 0.1), the
// pull-in before that a few loop time constants: 40 / bandwidth samples, rounded up to a power of two, covers both with margin
// (512 at 0.1; it was a fixed 1024).  Too short a warm-up only costs time: unmatched chunks are re-speculated / run serially.
static int costas_warm(float bandwidth) {
    const double want = 40.0 / std::max(1e-3, std::min(1.0, (double)fabsf(bandwidth)));
    int w = 256;
    while (w < want && w < 8192) w *= 2;
    return w;
}

// the loop's constants (everything of CostasArgs but the buffers)
static int costas_args(const urhgpu_params *p, CostasArgs &a) {
    a.noise_sqrd = p->noise_threshold * p->noise_threshold;
    // :253-254 as the reference's generated code evaluates them (damping = (float)(sqrt(2)/2), bandwidth*bandwidth a float product)
    const float bandwidth = p->costas_loop_bandwidth;
    const float damping = (float)(sqrt(2.0) / 2.0);
    const double den = (1.0 + ((2.0 * (double)damping) * (double)bandwidth)) + (double)(bandwidth * bandwidth);
    a.alpha = (float)(((4.0 * (double)damping) * (double)bandwidth) / den);
    a.beta = (float)(((4.0 * (double)bandwidth) * (double)bandwidth) / den);
    switch (p->dtype) {                                        // :267-283
        case URHGPU_DT_I8: a.scale = 127.5f; a.shift = 0.5f; break;
        case URHGPU_DT_U8: a.scale = 127.5f; a.shift = -127.5f; break;
        case URHGPU_DT_I16: a.scale = 32767.5f; a.shift = 0.5f; break;
        case URHGPU_DT_U16: a.scale = 65535.0f; a.shift = -32767.5f; break;
        case URHGPU_DT_F32: a.scale = 1.0f; a.shift = 0.0f; break;
        default: return URHGPU_ERR_DTYPE;
    }
    a.warm = costas_warm(bandwidth);
    int order = p->mod_order > 0 ? p->mod_order : (1 << p->bits_per_symbol);
    if (order > 4) order = 4;                                  // :285-287
    a.loop_order = order;
    return URHGPU_OK;
}

}  // namespace urh
