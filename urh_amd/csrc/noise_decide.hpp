// noise_decide.hpp -- the decision part of detect_noise_level (AutoInterpretation.py:74-91) on the chunks' float32 means and fp64 maxima,
// chunk 0 = the capture's last chunk, in the reference's own scalar types (filters.hip states them above k_noise_decide).  ONE definition,
// called by one thread of k_noise_decide (a capture alone: the statistics come from the chunk kernels) and by one thread of k_batch_noise
// (batch_auto.hip: a workgroup per capture computes the statistics itself), so that the two routes cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/urhgpu.h"

namespace urh {

// mean[k] = (float)(sum_k / chunk), mx[k] = the chunk's maximum (a NaN where the chunk holds one); any address space the caller has them in.
// use_cfg (a pass): where the value is not to be used -- flag 0, or flag 2: not below Signal.max_magnitude -- the block's noise_f32 /
// noise_sqrd are those of the configured threshold.
__device__ __forceinline__ urhgpu_noise_result noise_decide(const float *s_mean, const double *s_max, int64_t chunk, int n_chunks, double max_mag,
                                                            float cfg_noise, int use_cfg) {
    urhgpu_noise_result r;
    r.noise = 0.0; r.flag = 1; r.chunk = chunk; r.n_chunks = n_chunks; r.n_candidates = 0; r.min_mean = 0.0; r.max_mean = 0.0;
    if (n_chunks > 0) {
        float mn = s_mean[0], mxm = s_mean[0];
        bool nan = mn != mn;
        for (int k = 1; k < n_chunks; ++k) {
            const float e = s_mean[k];
            nan = nan || (e != e);
            if (e > mxm) mxm = e;
            if (e < mn) mn = e;
        }
        const double minimum = (double)mn, maximum = (double)mxm;
        r.min_mean = minimum; r.max_mean = maximum;
        if (!nan && !(maximum == 0.0 || minimum / maximum > 0.9)) {
            const float lim = 1.1f * mn;
            double result = 0.0;
            bool res_nan = false;
            int64_t cand = 0;
            for (int k = 0; k < n_chunks; ++k) {
                if (!(s_mean[k] <= lim)) continue;
                const double m = s_max[k];
                if (m != m) res_nan = true;
                if (cand == 0 || m > result) result = m;
                ++cand;
            }
            r.n_candidates = cand;
            if (cand > 0) {
                if (res_nan) result = __builtin_nan("");
                if (result != result || result == __builtin_inf() || result == -__builtin_inf()) { r.noise = result; r.flag = 0; }
                else r.noise = __builtin_ceil(result * 10000.0) / 10000.0;
            }
        }
    }
    if (r.flag == 1 && !(r.noise < max_mag)) r.flag = 2;
    r.noise_f32 = (use_cfg && r.flag != 1) ? cfg_noise : (float)r.noise;
    r.noise_sqrd = r.noise_f32 * r.noise_f32;
    return r;
}

}  // namespace urh
