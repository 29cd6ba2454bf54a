// batch_psk.hip -- the PSK demodulation of a batch of captures: a Costas loop PER CAPTURE, all of them in one launch (include/urhgpu.h
// "a batch of captures: PSK").
//
//   costa_demod   signal_functions.pyx:252-330, entered from afp_demod at :333-358
//
// The loop is a serial recurrence: about 94 dependent instructions per sample at about 9.5 cycles each (costas_prims.hpp, above
// costas_step_bf), of the order of 0.4 us per sample whatever else the machine does.  A pass over ONE capture hides that latency by cutting
// the capture into chunks and speculating on their start states (costas.hip); a short capture has no chunks to cut, and runs on one wavefront
// of the whole chip.  In a batch the parallelism is ACROSS captures: every capture starts in the known state {freq 0, phase 1.5}, nothing is
// speculated, and K loops run side by side.
//
//   k_batch_costas<DT, ORDER, DNOISE>   a LANE per capture, a wavefront (= a workgroup) per 64 captures taken in the plan's launch order
//       (longest first: the 64 lanes of a wavefront hold captures of similar length).  The loop body is costas_step_bf, straight-line code
//       written for one trajectory per lane; its `rare` ballot sends the whole wavefront through costas_step, which is exact for each lane's
//       own capture.  A lane past its capture's end is gated with an infinite threshold: its state is frozen, it takes no part in the ballot
//       and nothing of it is stored.
//       Per-lane strided loads and stores (lane r reading its capture's sample i: 64 cache lines per instruction) are staged through LDS in
//       tiles of 64 samples: for r = 0 .. 63 the wavefront loads 64 consecutive samples of capture r with ONE coalesced load into
//       tile_in[r][lane]; then 64 steps, in step u lane r reads tile_in[r][u] and writes tile_out[r][u]; then one coalesced store of row r's
//       valid part per r.  The row stride is 65 words (odd), so that the 64 reads of a step hit distinct banks.  No prefetch of the next
//       tile: a tile's 64 loads are issued 16 at a time and take a few microseconds against 64 x 0.4 us of steps.
// No workgroup waits for another; there are no atomics.  (The walk of a batch, k_batch_bits, is a wavefront per capture because its state
// machines are followed over the runs of a 64-sample step by ballot: there a lane per capture would serialise what the wavefront does in
// one instruction.  Here a step is one sample whatever the shape, and only the number of loops in flight counts.)
#include "batch_kernels.hpp"      // (first: the fp64 forms of URH_FDIV / URH_FSQRT)

#include <algorithm>

#include "costas_prims.hpp"

namespace urh {

constexpr int kBcTile = 64;                // samples per tile = captures per wavefront
constexpr int kBcStride = kBcTile + 1;     // row stride in words: odd, the lanes of a step read distinct banks
constexpr int kBcLoads = 16;               // coalesced loads in flight while a tile is filled

template <int DT, int ORDER, bool DNOISE>
__global__ __launch_bounds__(64) void k_batch_costas(const CostasArgs a0, const BatchArgs b, const urhgpu_noise_result *d_noise) {
    __shared__ float2 tile_in[kBcTile * kBcStride];        // 33 280 bytes
    __shared__ float tile_out[kBcTile * kBcStride];        // 16 640 bytes
    __shared__ int64_t s_s0[kBcTile];                      // row r: its capture's first sample ...
    __shared__ int s_n[kBcTile];                           // ... and the samples its loop covers (0: none)
    const int lane = (int)threadIdx.x;
    const int64_t slot = (int64_t)blockIdx.x * kBcTile + lane;

    // ---- my capture: afp_demod's rules (k_batch_demod, batch_center.hip) ----
    int64_t s0 = 0;
    int n_loop = 0;                                        // the loop runs over samples 1 .. n_loop - 1
    float nsq = a0.noise_sqrd;
    if (slot < b.k) {
        const int64_t c = b.plan[2 * b.k + slot];          // launch order: longest capture first
        if (c >= 0 && c < b.k) {
            const BatchCapture cap = batch_capture(b, c);  // (n is the samples' alone: a refused start or end is an empty capture)
            bool two = false;
            if (DNOISE) {
                const urhgpu_noise_result *r = d_noise + c;
                nsq = r->noise_sqrd;
                two = r->flag == 2 && cap.n > 2;
            }
            const int n = two ? 2 : (int)cap.n;            // < 2^31
            s0 = cap.s0;
            float *q = b.qad + s0;
            if (n <= 2) {                                  // :335-336
                for (int i = 0; i < n; ++i) q[i] = 0.0f;
            } else {
                q[0] = -4.0f;                              // reference: np.empty, never written (documented in urhgpu.h)
                n_loop = n;
            }
        }
    }
    s_s0[lane] = s0;
    s_n[lane] = n_loop;
    int n_max = n_loop;                                    // the wavefront's longest loop
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_max = max(n_max, __shfl_xor(n_max, o));
    n_max = __builtin_amdgcn_readfirstlane(n_max);
    __syncthreads();

    CostasState st{0.0f, 1.5f};                            // :261; never crosses a capture boundary
    float err = 0.0f;
    // (sample indices are unsigned 32-bit: a capture holds up to 2^31 - 1 samples, and base + 64 must not wrap for the longest of them)
    const uint32_t n_end = (uint32_t)n_max, n_mine = (uint32_t)n_loop;
    for (uint32_t base = 0; base < n_end; base += kBcTile) {
        const uint32_t i_l = base + (uint32_t)lane;        // the sample of a row this lane loads and stores
        // ---- fill: row r = 64 consecutive samples of capture r, one coalesced load each, kBcLoads of them in flight ----
#pragma unroll 1
        for (int r0 = 0; r0 < kBcTile; r0 += kBcLoads) {
            if (base >= (uint32_t)__builtin_amdgcn_readfirstlane(s_n[r0])) {
                // (rows in launch order end from the back; a plan that is not sorted only loses this shortcut for the rows behind)
                bool any = false;
                for (int j = 1; j < kBcLoads; ++j) any |= base < (uint32_t)__builtin_amdgcn_readfirstlane(s_n[r0 + j]);
                if (!any) continue;
            }
            float2 v[kBcLoads];
#pragma unroll
            for (int j = 0; j < kBcLoads; ++j) {
                const uint32_t nr = (uint32_t)s_n[r0 + j];
                v[j] = make_float2(0.0f, 0.0f);
                if (i_l < nr) v[j] = CostasLoad<DT>::at(b.iq, s_s0[r0 + j] + (int64_t)i_l);
            }
#pragma unroll
            for (int j = 0; j < kBcLoads; ++j) tile_in[(r0 + j) * kBcStride + lane] = v[j];
        }
        __syncthreads();
        // ---- 64 steps: lane r follows capture r ----
        const int steps = (n_end - base < (uint32_t)kBcTile) ? (int)(n_end - base) : kBcTile;
#pragma unroll 1
        for (int u = 0; u < steps; ++u) {
            const uint32_t i = base + (uint32_t)u;
            const bool active = i >= 1 && i < n_mine;      // the loop starts at sample 1 (:289)
            float2 sm = tile_in[lane * kBcStride + u];
            CostasArgs a = a0;
            // a lane whose capture has ended (or has no loop): gated whatever lies in the tile -- state frozen, no part in the `rare` ballot
            a.noise_sqrd = active ? nsq : __builtin_inff();
            sm = active ? sm : make_float2(0.0f, 0.0f);
            tile_out[lane * kBcStride + u] = costas_step_bf<DT == URHGPU_DT_F32, ORDER>(sm, st, err, a);
        }
        __syncthreads();
        // ---- drain: one coalesced store of row r's valid part ----
#pragma unroll 4
        for (int r = 0; r < kBcTile; ++r) {
            const uint32_t nr = (uint32_t)s_n[r];
            if (i_l >= 1 && i_l < nr) b.qad[s_s0[r] + (int64_t)i_l] = tile_out[r * kBcStride + lane];
        }
        __syncthreads();                                   // (the next fill rewrites the tiles)
    }
}

// PSK parameters a batch accepts: batch_check_params_psk's, and a loop order the reference writes an output for
int batch_costas_check(const urhgpu_params *p) {
    URH_TRY(batch_check_params_psk(p));
    CostasArgs a;
    URH_TRY(costas_args(p, a));
    return (a.loop_order == 2 || a.loop_order == 4) ? URHGPU_OK : URHGPU_ERR_UNSUPPORTED;
}

// ONE launch: the Costas loop of every capture of b into b.qad (p has passed batch_costas_check; of b the samples, starts, plan, k, total
// and qad are read -- batch_capture vouches for the samples alone)
int launch_batch_costas(const urhgpu_params *p, const BatchArgs &b, const urhgpu_noise_result *d_noise, hipStream_t s) {
    CostasArgs a;
    a.iq = b.iq; a.n = b.total; a.out = b.qad;
    URH_TRY(costas_args(p, a));
    const unsigned grid = (unsigned)std::max<int64_t>((b.k + kBcTile - 1) / kBcTile, 1);
    return dispatch_dtype(p->dtype, [&](auto dt) {
        // (any other loop order: the reference leaves the output unwritten)
        return dispatch_one_of<2, 4>(a.loop_order, URHGPU_ERR_UNSUPPORTED, [&](auto order) {
            return dispatch_bool(d_noise != nullptr, [&](auto dn) {
                hipLaunchKernelGGL((k_batch_costas<dt.value, order.value, dn.value>), dim3(grid), dim3(64), 0, s, a, b, d_noise);
                return URHGPU_OK;
            });
        });
    });
}

}  // namespace urh

using namespace urh;

extern "C" {

int urhgpu_batch_costas_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                            const urhgpu_params *p, const urhgpu_noise_result *d_noise, float *d_qad) {
    if (!ctx || k < 0 || k > INT32_MAX || total < 0) return URHGPU_ERR_ARG;
    URH_TRY(batch_costas_check(p));
    if (k > 0 && (!d_start || !d_plan)) return URHGPU_ERR_ARG;
    if ((total > 0 && (!d_iq || !d_qad)) || ((uintptr_t)d_iq & 15) || ((uintptr_t)d_qad & 3)) return URHGPU_ERR_ARG;
    if (((uintptr_t)d_start & 7) || ((uintptr_t)d_plan & 7) || ((uintptr_t)d_noise & 7)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    BatchArgs b;
    memset(&b, 0, sizeof(b));                              // no work buffer: batch_capture then vouches for the samples alone
    b.iq = d_iq; b.start = d_start; b.plan = d_plan; b.k = k; b.total = total; b.qad = d_qad;
    b.sps = p->samples_per_symbol; b.bps = p->bits_per_symbol; b.tol = p->tolerance;
    URH_TRY(launch_batch_costas(p, b, d_noise, ctx->stream));
    ctx->batch_launches += 1;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

}  // extern "C"
