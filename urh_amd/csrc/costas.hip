// costas.hip -- the Costas-loop PSK demodulator (row 5 of SURVEY.md §8a) for gfx950.
//
//   costa_demod   /root/reference/src/urh/cythonext/signal_functions.pyx:252-330
//
// The loop is a nonlinear recurrence over the whole capture: state (freq, phase) in float32, per step a noise gate,
// sinf / cosf of the phase (glibc's, restated in glibc_sincosf.h), a complex product, a clamped error, two state
// updates, a wrap into +-2*pi evaluated in double.  Every output must equal the serial evaluation bit for bit.
//
// Exact parallel evaluation (k_costas_spec / k_costas_map / k_costas_stitch / k_costas_final):
//   * The capture is cut into chunks of kChunk samples.  Started from ANY state, the loop forgets that state: after
//     some hundred un-gated samples two trajectories that lock onto the same phase ambiguity become bit-identical
//     (measured on the reference).  The lock points are pi/2 (order 4) or pi (order 2) apart, each with a
//     twin 2*pi away inside the +-2*pi wrap range.
//   * k_costas_spec runs, for every chunk, one candidate per lock point: it starts `warm` un-gated samples before the
//     chunk from phase 1.5 + k * (pi/2 | pi), freq 0, and records the candidate's state at the chunk start (S), at
//     checkpoints inside the chunk (CP) and at its end (E).  Chunk 0's candidate 0 IS the true trajectory.
//   * k_costas_map: for every chunk c and candidate k of chunk c-1, which candidate of chunk c starts (bitwise) in
//     E[c-1][k]?  k_costas_stitch follows this map from chunk 0: as long as a candidate matches, the true state at
//     the next chunk start is known without touching a sample.  Where nothing matches (acquisition, long gated
//     stretches) it evaluates the chunk serially from the true state, leaving it as soon as the state equals a
//     candidate's checkpoint.  Either way the TRUE state at every chunk start comes out.
//   * k_costas_final re-evaluates every chunk from its true start state, in parallel, and writes the output.  (Tried in round 3:
//     the candidate pass keeps every distinct candidate's output -- collected 16 samples at a time, written as whole 64-byte lines into
//     a slot per candidate -- and a gather kernel copies the true candidate's slot per chunk, so that this pass only re-evaluates
//     chunks without one.  Bit-identical, but no faster: the candidate pass grew from 1.96 to 2.22 ms, the gather took 0.23, against
//     0.69 saved here: 3.36 instead of 3.39 ms per 2^27 samples, for 2 GB more scratch.  Not kept.)
// The result is exact by construction (equality is tested on the state bits, never assumed); only the speed depends on
// how quickly candidates converge.  Work: (K warm + D kChunk + kChunk) steps per chunk instead of kChunk (D <= K distinct candidates).
// Loop orders other than 2 and 4 leave the output unwritten in the reference; they use the serial kernel.
//
// Bound: dependent-instruction latency, hidden by running one chunk-candidate per lane over the whole machine.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <math.h>
#include <string.h>
#include <type_traits>

#include "cmul.hpp"
#include "common.hpp"
#include "costas_prims.hpp"
#include "dispatch.hpp"
#include "launchers.hpp"
#include "glibc_sincosf.h"

namespace urh {

// One rank's shard of a sharded capture (the SH instantiations below; include/urhgpu.h, "PSK across shards"): local sample i is
// global sample pos_base + i, and the raw samples handed over with the shard (its left halo) are local samples -n_halo .. -1.
// Chunks are laid out from the shard's start.
struct CostasArgsSh : CostasArgs {
    const void *halo_end;    // one past the halo: local sample i < 0 is read at halo_end[i] (nullptr on rank 0)
    int64_t origin;          // first sample of chunk 0: 1 on rank 0 (global sample 0 is not part of the loop), 0 on the others
    int64_t lo;              // lowest local sample a walk back reads: max(1 - pos_base, -n_halo)
    int64_t start1;          // local index of global sample 1, where the loop starts in {0, 1.5}: 1 - pos_base
};
template <bool SH> using CostasArgsT = typename std::conditional<SH, CostasArgsSh, CostasArgs>::type;

template <class A>
__device__ __forceinline__ A costas_device_noise(const A &a_in) {
    A a = a_in;
    if (a.d_noise) a.noise_sqrd = *a.d_noise;                  // (a uniform load, once per workgroup)
    return a;
}
// ---- serial evaluation: one wavefront, every lane the same recurrence, lane k keeps outputs k, k+64, ... of a tile ----
constexpr int kCostasTile = 1024;

template <int DT>
__global__ __launch_bounds__(64) void k_costas(const CostasArgs a_in) {
    const CostasArgs a = costas_device_noise(a_in);
    __shared__ float2 s_x[kCostasTile];
    const int lane = threadIdx.x;
    CostasState st{0.0f, 1.5f};                                // :261
    float err = 0.0f;
    if (lane == 0 && a.n > 0) a.out[0] = -4.0f;                // reference: np.empty, never written (documented in urhgpu.h)
    for (int64_t base = 0; base < a.n; base += kCostasTile) {
        const int tv = (int)((a.n - base < kCostasTile) ? (a.n - base) : kCostasTile);
        __syncthreads();
        for (int u = lane; u < tv; u += 64) s_x[u] = CostasLoad<DT>::at(a.iq, base + u);
        __syncthreads();
        float mine[kCostasTile / 64];
#pragma unroll 1
        for (int g = 0; g < kCostasTile / 64; ++g) {
            float keep = 0.0f;
#pragma unroll 1
            for (int u = 0; u < 64; ++u) {
                const int k = g * 64 + u;
                if (k >= tv || (base + k) == 0) continue;       // the loop starts at sample 1 (:289)
                const float o = costas_step<DT == URHGPU_DT_F32>(s_x[k], st, err, a);
                if (u == lane) keep = o;
            }
            mine[g] = keep;
        }
#pragma unroll 1
        for (int g = 0; g < kCostasTile / 64; ++g) {
            const int k = g * 64 + lane;
            if (k < tv && base + k != 0) a.out[base + k] = mine[g];
        }
    }
}

// ---- speculative parallel evaluation ----------------------------------------------------------------------------------
// samples per chunk.  Round 3, config-5 capture (tools/costas_chunk_ab.py, libraries built with -DURH_COSTAS_CHUNK=...): 1024 / 2048 / 4096 /
// 8192 samples per chunk take 5.04 / 3.83 / 3.39 / 3.92 ms -- shorter chains, but as many warm-up steps per chunk as before.
#ifndef URH_COSTAS_CHUNK
#define URH_COSTAS_CHUNK 4096
#endif
constexpr int kChunk = URH_COSTAS_CHUNK;
constexpr int kWarmBackFactor = 16; // a candidate looks back at most 16 x its warm-up length for un-gated samples
constexpr int kCkpt = 256;          // checkpoint spacing inside a chunk
constexpr int kNumCkpt = kChunk / kCkpt;   // checkpoints at offsets kCkpt, 2 kCkpt, ... < kChunk  (index j = off / kCkpt - 1)
constexpr int kMaxCand = 8;

struct SpecBuffers {
    CostasState *S;        // [n_chunks][K]  state at the chunk start (before its first sample)
    CostasState *E;        // [n_chunks][K]  state after the chunk's last sample
    CostasState *CP;       // [n_chunks][kNumCkpt][K] state after offset (j+1)*kCkpt samples of the chunk
    uint32_t *map;         // [n_chunks] nibble k: candidate of this chunk that starts in E[c-1][k], 0xF none
    CostasState *T;        // [n_chunks] TRUE state at the chunk start (written by the stitch)
    int32_t *run_list;     // [n_chunks * K] chunk * K + candidate of every DISTINCT candidate (k_costas_spec appends, k_costas_run consumes)
    int32_t *run_count;    // [1] entries in run_list
    uint8_t *is_rep;       // [n_chunks][K] 1: the candidate runs (no lower-numbered candidate of the chunk starts in the same state)
    int32_t *gidx;         // [n_chunks] candidate whose trajectory IS the true one over the whole chunk, or -1 (written by the stitch)
    int32_t *ungated;      // [n_chunks] un-gated samples in the chunk
    CostasState *resume;   // [1] true state at the start of chunk stats[3] when the stitch hands back to the host
    int32_t *stats;        // [0] chunks resolved by the map, [1] by a checkpoint inside a serial run, [2] fully serial,
                           // [3] chunk the stitch stopped in front of (n_chunks: finished), [4] re-speculation rounds;
                           // 64 bytes further on: the device-driven loop's control block (costas_ctl)
};
// What the host-driven loop (launch_costas_spec) learns from the stitch and hands to the next round's kernels as arguments, kept on the
// device instead: the DEV instantiations of the round kernels read it, their stitch rewrites it on exit -- a break stores the next round's
// {c_from, use_seed = 1, seed_freq = the true loop's frequency there} and counts the round, a closed chain sets `done`, and every round
// kernel queued behind that returns on this one load.  Zeroed with the stats (one memset): round 0 is {c_from 0, no seed, not done}.
struct CostasCtl {
    int64_t c_from;
    int32_t use_seed;
    float seed_freq;
    int32_t done;
    int32_t rounds;
};
// (no pointer of its own in SpecBuffers: the stitch keeps b.stats to its last instruction anyway, a second one cost it two more scalar registers)
__host__ __device__ __forceinline__ CostasCtl *costas_ctl(const SpecBuffers &b) { return (CostasCtl *)(b.stats + 16); }

__device__ __forceinline__ bool same_state(CostasState a, CostasState b) {
    return __float_as_uint(a.freq) == __float_as_uint(b.freq) && __float_as_uint(a.phase) == __float_as_uint(b.phase);
}
__device__ __forceinline__ int64_t chunk_begin(int64_t c) { return 1 + c * (int64_t)kChunk; }   // sample 0 is not part of the loop

// What the SH (shard) instantiations read from CostasArgsSh; the single-GPU instantiations keep the constants of a whole capture.
template <bool SH, class A> __device__ __forceinline__ int64_t chunk_begin_of(const A &a, int64_t c) {
    if constexpr (SH) return a.origin + c * (int64_t)kChunk;
    else return chunk_begin(c);
}
template <int DT, bool SH, class A> __device__ __forceinline__ float2 costas_at(const A &a, int64_t i) {
    if constexpr (SH) return CostasLoad<DT>::at(i < 0 ? a.halo_end : a.iq, i);      // the halo: local samples < 0
    else return CostasLoad<DT>::at(a.iq, i);
}
template <bool SH, class A> __device__ __forceinline__ int64_t walk_floor(const A &a) {
    if constexpr (SH) return a.lo;
    else return 1;
}
template <bool SH, class A> __device__ __forceinline__ int64_t loop_start(const A &a) {
    if constexpr (SH) return a.start1;
    else return 1;
}
template <bool SH, class A> __device__ __forceinline__ bool chunk0_exact(const A &a) {     // chunk 0 starts where the loop does
    if constexpr (SH) return a.origin == 1;
    else return true;
}

// Candidates of the chunks c >= c_from.  use_seed: all candidates start with freq = seed_freq (the true loop's own
// frequency where the chain last broke) instead of the estimate from the data.
// SH (a shard): the walk back reads into the halo and stops at global sample 1, exactly where the single-GPU walk does.
// DEV: c_from / use_seed / seed_freq come from the control block (the arguments are ignored), nothing to do once the chain has closed.
template <int DT, int ORDER, bool SH = false, bool DEV = false>
__global__ __launch_bounds__(256) void k_costas_spec(const CostasArgsT<SH> a_in, SpecBuffers b, int64_t n_chunks, int K, int64_t c_from,
                                                      int use_seed, float seed_freq) {
    const CostasArgsT<SH> a = costas_device_noise(a_in);
    if constexpr (DEV) {
        if (costas_ctl(b)->done) return;
        c_from = costas_ctl(b)->c_from; use_seed = costas_ctl(b)->use_seed; seed_freq = costas_ctl(b)->seed_freq;
    }
    const int64_t gid = blockIdx.x * 256ll + threadIdx.x;
    const int64_t c = c_from + gid / K;
    const int k = (int)(gid % K);
    if (c >= n_chunks) return;
    const int64_t s0 = chunk_begin_of<SH>(a, c);
    // candidate k: phase 1.5 + (k - K/2) * spacing, spaced pi/2 (order 4, K = 8) or pi (order 2, K = 4): every lock point and its
    // twin 2*pi away; candidate K/2 has the reference's own initial phase 1.5
    const float spacing = (a.loop_order == 4) ? 1.57079632679489661923f : 3.14159265358979323846f;
    CostasState st{0.0f, 1.5f + (float)(k - K / 2) * spacing};
    float err = 0.0f;
    int64_t p = s0;
    if (c == 0 && chunk0_exact<SH>(a)) {
        st = CostasState{0.0f, 1.5f};                       // every candidate of chunk 0 is the true trajectory
    } else {
        int ungated = 0;
        const int64_t back = (int64_t)kWarmBackFactor * a.warm;
        const int64_t floor = walk_floor<SH>(a);
        // walk back until `warm` un-gated samples lie between p and the chunk -- eight samples per round trip to memory
        while (p > floor && ungated < a.warm && s0 - p < back) {
            float2 g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = costas_at<DT, SH>(a, (p - 1 - j >= floor) ? p - 1 - j : floor);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (p > floor && ungated < a.warm && s0 - p < back) {
                    --p;
                    if (!costas_gated(g[j], a)) ++ungated;
                }
            }
        }
        if (p == loop_start<SH>(a)) {
            st = CostasState{0.0f, 1.5f};                   // reached the start of the capture: exact, not a guess
        } else if (use_seed) {
            st.freq = seed_freq;
        } else {
            // Seed the candidate's frequency with the carrier offset of the warm-up stretch (M-th power of the
            // differential phase: the PSK symbol steps are multiples of 2*pi/M and drop out).  A candidate that starts
            // at freq 0 against an offset beyond the loop bandwidth needs thousands of samples to pull in; seeded, it
            // locks within the warm-up.  Heuristic only: a wrong seed costs time (serial fallback), never exactness.
            float ax = 0.0f, ay = 0.0f;
            float2 prev = costas_at<DT, SH>(a, p);
            bool prev_ok = !costas_gated(prev, a);
            const int64_t wend = (p + 512 < s0) ? p + 512 : s0;
            for (int64_t i0 = p + 1; i0 < wend; i0 += 8) {
                float2 g[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) g[j] = costas_at<DT, SH>(a, (i0 + j < wend) ? i0 + j : wend - 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (i0 + j < wend) {
                        const float2 cur = g[j];
                        const bool ok = !costas_gated(cur, a);
                        if (ok && prev_ok) {
                            const float cr = (cur.x + a.shift) / a.scale, ci = (cur.y + a.shift) / a.scale;
                            const float pr = (prev.x + a.shift) / a.scale, pi = (prev.y + a.shift) / a.scale;
                            float dx = cr * pr + ci * pi, dy = ci * pr - cr * pi;          // cur * conj(prev)
                            float tx = dx * dx - dy * dy, ty = 2.0f * dx * dy;             // ^2
                            if (a.loop_order == 4) { const float ux = tx * tx - ty * ty, uy = 2.0f * tx * ty; tx = ux; ty = uy; }
                            ax += tx; ay += ty;
                        }
                        prev = cur; prev_ok = ok;
                    }
                }
            }
            if (ax != 0.0f || ay != 0.0f) st.freq = costas_clamp(atan2f(ay, ax) / (float)a.loop_order);
        }
        {
            constexpr int PF = 4;                               // as in k_costas_run: the next four samples are on their way
            float2 cur[PF];
#pragma unroll
            for (int j = 0; j < PF; ++j) cur[j] = costas_at<DT, SH>(a, (p + j < s0) ? p + j : s0 - 1);
            for (int64_t i = p; i < s0; i += PF) {
                float2 nxt[PF];
#pragma unroll
                for (int j = 0; j < PF; ++j) { const int64_t q = i + PF + j; nxt[j] = costas_at<DT, SH>(a, (q < s0) ? q : s0 - 1); }
#pragma unroll
                for (int j = 0; j < PF; ++j) if (i + j < s0) costas_step_bf<DT == URHGPU_DT_F32, ORDER>(cur[j], st, err, a);
#pragma unroll
                for (int j = 0; j < PF; ++j) cur[j] = nxt[j];
            }
        }
    }
    b.S[c * K + k] = st;
    // Candidates that have met during the warm-up -- the twins 2*pi apart do as soon as a carrier offset has wrapped the
    // phase once, every candidate of chunk 0 is the true trajectory -- would repeat each other sample for sample: only
    // the lowest-numbered one of every distinct start state runs the chunk (k_costas_run, lanes packed densely).
    const int lane = threadIdx.x & 63, base = lane - k;              // the chunk's K candidates are adjacent lanes of one wavefront
    bool dup = false;
    for (int j = 0; j < K; ++j) {
        CostasState o;
        o.freq = __shfl(st.freq, base + j); o.phase = __shfl(st.phase, base + j);
        if (j < k && same_state(o, st)) dup = true;
    }
    b.is_rep[c * K + k] = dup ? 0 : 1;
    const unsigned long long m = __ballot(!dup);
    int pos = 0;
    if (lane == __builtin_ctzll(m)) pos = atomicAdd(b.run_count, __builtin_popcountll(m));
    pos = __shfl(pos, __builtin_ctzll(m));
    if (!dup) b.run_list[pos + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int32_t)(c * K + k);
}

// The chunk itself, one lane per distinct candidate: checkpoints, end state, un-gated sample count.
template <int DT, int ORDER, bool SH = false>
__global__ __launch_bounds__(256) void k_costas_run(const CostasArgsT<SH> a_in, SpecBuffers b, int K) {
    const CostasArgsT<SH> a = costas_device_noise(a_in);
    const int64_t gid = blockIdx.x * 256ll + threadIdx.x;
    if (gid >= *b.run_count) return;
    const int64_t ck = b.run_list[gid];
    const int64_t c = ck / K;
    const int k = (int)(ck % K);
    const int64_t s0 = chunk_begin_of<SH>(a, c);
    const int64_t e0 = (s0 + kChunk < a.n) ? s0 + kChunk : a.n;
    CostasState st = b.S[ck];
    float err = 0.0f;
    int ung = 0;
    // The samples of the NEXT four steps are requested before the current four are evaluated: a step is ~130 dependent instructions,
    // and with two wavefronts per SIMD (one lane per distinct candidate) nothing else hides the latency of its own load -- half of
    // the wave cycles were spent in s_waitcnt before.
    constexpr int PF = 4;
    float2 cur[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) cur[j] = CostasLoad<DT>::at(a.iq, (s0 + j < e0) ? s0 + j : e0 - 1);
    for (int64_t i = s0; i < e0; i += PF) {
        float2 nxt[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) { const int64_t q = i + PF + j; nxt[j] = CostasLoad<DT>::at(a.iq, (q < e0) ? q : e0 - 1); }
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            if (i + j < e0) {
                if (!costas_gated(cur[j], a)) ++ung;
                costas_step_bf<DT == URHGPU_DT_F32, ORDER>(cur[j], st, err, a);
                const int off = (int)(i + j - s0) + 1;
                if (off % kCkpt == 0 && off < kChunk) b.CP[(c * kNumCkpt + (off / kCkpt - 1)) * K + k] = st;
            }
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) cur[j] = nxt[j];
    }
    b.E[ck] = st;
    if (k == 0) b.ungated[c] = ung;
}

template <bool DEV = false>
__global__ __launch_bounds__(256) void k_costas_map(SpecBuffers b, int64_t n_chunks, int K, int64_t c_from) {
    if constexpr (DEV) {
        if (costas_ctl(b)->done) return;
        c_from = costas_ctl(b)->c_from > 1 ? costas_ctl(b)->c_from : 1;
    }
    const int64_t c = c_from + blockIdx.x * 256ll + threadIdx.x;
    if (c >= n_chunks) return;
    uint32_t m = 0xFFFFFFFFu;
    if (c > 0) {
        for (int k = 0; k < K; ++k) {
            int hit = 0xF;
            if (b.is_rep[(c - 1) * K + k]) {                 // a duplicate did not run: no end state (it is never the carrying candidate)
                const CostasState e = b.E[(c - 1) * K + k];
                for (int q = 0; q < K; ++q) if (same_state(e, b.S[c * K + q])) { hit = q; break; }
            }
            m = (m & ~(0xFu << (4 * k))) | ((uint32_t)hit << (4 * k));
        }
    }
    b.map[c] = m;
}

// Composition of two chunk maps (8 nibbles: candidate of the previous chunk -> candidate of this chunk, 0xF = none):
// (later o earlier)[k] = later[earlier[k]], none stays none.
__device__ __forceinline__ uint32_t map_compose(uint32_t later, uint32_t earlier) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t mid = (earlier >> (4 * k)) & 0xFu;
        const uint32_t v = (mid == 0xFu) ? 0xFu : ((later >> (4 * mid)) & 0xFu);
        r |= v << (4 * k);
    }
    return r;
}

// One wavefront walks the chunks c_from .. in order.  While a candidate carries the true trajectory the walk is a
// composition of the chunk maps, evaluated 1024 chunks at a time (16 per lane) by a wavefront prefix "scan" with map_compose (the serial
// walk -- two dependent global loads per chunk -- took 10.9 ms for the 32 767 chunks of a 1 GiB capture).  Where the maps
// end (acquisition, long gated stretches) the chunk is handled as before: compare the true state with the chunk's
// candidates, else evaluate it serially from the true state until it meets a candidate at a checkpoint.
// Entry: the true state at the start of chunk c_from is *b.resume (c_from == 1: chunk 0's end, taken from E[0][0]).
// Exit: either all chunks are resolved, or -- when allow_break -- the chain broke for good (a chunk with plenty of
// un-gated samples was evaluated serially to its end and met no candidate): stats[3] = the next chunk, *b.resume = its true
// start state, and the host re-speculates the remaining chunks around that state's frequency.
// SH (a shard): chunk 0 is never taken as exact -- the walk starts at c_from from the true state *b.resume, for c_from == 0 the
// state the ranks before this one hand over -- and the true state after the shard's last sample is left in b.resume[1].
constexpr int kStitchBlock = 1024;              // 16 wavefronts: the fast-forward composes 4096 chunk maps per round
// DEV: c_from comes from the control block, which the exit rewrites for the round queued behind this one (see CostasCtl); the host
// passes allow_break = 0 to the last stitch it has queued, so the chain always closes.
template <int DT, int ORDER, bool SH = false, bool DEV = false>
__global__ __launch_bounds__(kStitchBlock) void k_costas_stitch(const CostasArgsT<SH> a_in, SpecBuffers b, int64_t n_chunks, int K, int64_t c_from,
                                                                 int allow_break) {
    const CostasArgsT<SH> a = costas_device_noise(a_in);
    if constexpr (DEV) {
        const int done = costas_ctl(b)->done;
        c_from = costas_ctl(b)->c_from > 1 ? costas_ctl(b)->c_from : 1;
        __syncthreads();                            // (every thread has read the block before thread 0 may rewrite it)
        if (done) return;
    }
    __shared__ uint32_t s_wp[kStitchBlock / 64];    // per-wavefront composition of its chunk maps
    __shared__ int s_fail, s_cand, s_flags;         // first position where the chain ends; broadcast slots
    __shared__ CostasState s_T;
    __shared__ long long s_c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cand = -1;                                  // candidate of chunk c - 1 that is the true trajectory, or -1
    CostasState T = *b.resume;                      // true state at the start of chunk c (valid while cand < 0)
    if (!SH && c_from == 1) { cand = 0; if (tid == 0) { b.T[0] = CostasState{0.0f, 1.5f}; b.gidx[0] = 0; } }   // chunk 0: every candidate is exact
    int n_map = 0, n_ckpt = 0, n_serial = 0;        // (kept identically by every thread in the fast-forward, by wavefront 0 below)
    int64_t stop_at = n_chunks;
    int64_t c = c_from;
    bool map_failed = false;                        // chunk c: the map already said that no candidate starts in T
    bool stop = false;
    while (c < n_chunks && !stop) {
        while (cand >= 0 && c < n_chunks) {         // ---- fast-forward over up to 4096 chunks: 4 consecutive chunks per thread
            constexpr int Q = 4;
            if (tid == 0) s_fail = 0x7fffffff;
            const int64_t cc0 = c + (int64_t)Q * tid;
            uint32_t L[Q];                                            // L[q] = map[cc0 + q] o ... o map[cc0]
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const uint32_t m = (cc0 + q < n_chunks) ? b.map[cc0 + q] : 0xFFFFFFFFu;
                L[q] = q ? map_compose(m, L[q - 1]) : m;
            }
            uint32_t P = L[Q - 1];                                    // inclusive prefix composition over the lanes of the wavefront
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(P, o);
                if (lane >= o) P = map_compose(P, u);
            }
            if (lane == 63) s_wp[wave] = P;
            __syncthreads();
            uint32_t X = 0x76543210u;                                 // everything before my first chunk: the wavefronts before mine ...
            for (int w = 0; w < wave; ++w) X = map_compose(s_wp[w], X);
            const uint32_t before = __shfl_up(P, 1);                  // ... then the lanes before me
            if (lane != 0) X = map_compose(before, X);
            uint32_t g[Q], gp[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) g[q] = (map_compose(L[q], X) >> (4 * cand)) & 0xFu;   // candidate of chunk cc0 + q on the true trajectory
            gp[0] = (X >> (4 * cand)) & 0xFu;
#pragma unroll
            for (int q = 1; q < Q; ++q) gp[q] = g[q - 1];
            CostasState Tl[Q];
            int firstq = Q;                                           // my first chunk where the chain ends
#pragma unroll
            for (int q = Q - 1; q >= 0; --q) {
                const int64_t cc = cc0 + q;
                const bool reach = (gp[q] != 0xFu) && (cc < n_chunks);   // the true state at the start of chunk cc is E[cc - 1][gp]
                Tl[q] = T;
                if (reach) { Tl[q] = b.E[(cc - 1) * K + gp[q]]; b.T[cc] = Tl[q]; b.gidx[cc] = (g[q] == 0xFu) ? -1 : (int32_t)g[q]; }
                if (reach && g[q] == 0xFu) firstq = q;
            }
            if (firstq < Q) atomicMin(&s_fail, tid * Q + firstq);
            __syncthreads();
            const int fail = s_fail;
            const int64_t left = n_chunks - c;
            const int total = (int)(left < (int64_t)kStitchBlock * Q ? left : (int64_t)kStitchBlock * Q);
            const int pos = (fail == 0x7fffffff) ? total - 1 : fail;      // the chunk whose thread has the hand-over value
            if (tid == pos / Q) {
                const int qq = pos % Q;
                uint32_t gl = g[0];
                CostasState Ts = Tl[0];
#pragma unroll
                for (int q = 1; q < Q; ++q) if (qq == q) { gl = g[q]; Ts = Tl[q]; }
                s_cand = (int)gl; s_T = Ts;
            }
            __syncthreads();
            if (fail == 0x7fffffff) {
                cand = s_cand;
                n_map += total; c += total;
            } else {
                T = s_T;
                n_map += fail; c += fail; cand = -1; map_failed = true;
            }
            __syncthreads();                                          // (s_fail / s_cand / s_T are rewritten by the next round)
        }
        if (c >= n_chunks) break;
        // ---- chunk c without a carrying candidate: T is the true state at its start.  One wavefront's work; the others wait.
        if (wave == 0) {
            bool done = false;
            if (!map_failed) {
                if (lane == 0) { b.T[c] = T; b.gidx[c] = -1; }
                const bool hit = lane < K && same_state(T, b.S[c * K + lane]);
                const unsigned long long m = __ballot(hit);
                if (m) {
                    cand = __builtin_ctzll(m);
                    if (lane == 0) b.gidx[c] = cand;
                    ++n_map; ++c;
                    done = true;
                }
            }
            if (!done) {
                map_failed = false;
                if (b.ungated[c] == 0) { ++n_serial; ++c; done = true; }     // fully gated chunk: the state does not move
            }
            if (!done) {
                // no candidate starts in T: evaluate the chunk from T until the state meets a candidate at a checkpoint
                const int64_t s0 = chunk_begin_of<SH>(a, c);
                const int64_t e0 = (s0 + kChunk < a.n) ? s0 + kChunk : a.n;
                float err = 0.0f;
                CostasState st = T;
                for (int64_t i = s0; i < e0; ++i) {
                    costas_step_bf<DT == URHGPU_DT_F32, ORDER>(CostasLoad<DT>::at(a.iq, i), st, err, a);
                    const int off = (int)(i - s0) + 1;
                    if (off % kCkpt == 0 && off < kChunk) {
                        const bool hit = lane < K && b.is_rep[c * K + lane] && same_state(st, b.CP[(c * kNumCkpt + (off / kCkpt - 1)) * K + lane]);
                        const unsigned long long m = __ballot(hit);
                        if (m) { cand = __builtin_ctzll(m); break; }
                    }
                }
                if (cand >= 0) { ++n_ckpt; ++c; }       // gidx[c] stays -1: only part of the chunk lies on the candidate
                else {
                    ++n_serial;
                    T = st;                             // the state at the END of chunk c = start of chunk c + 1
                    if (allow_break && b.ungated[c] >= kChunk / 2 && c + 1 < n_chunks) { stop_at = c + 1; stop = true; }
                    else ++c;
                }
            }
            if (lane == 0) { s_c = c; s_cand = cand; s_T = T; s_flags = (map_failed ? 1 : 0) | (stop ? 2 : 0); }
        }
        __syncthreads();
        c = s_c; cand = s_cand; T = s_T; map_failed = (s_flags & 1) != 0; stop = (s_flags & 2) != 0;
        __syncthreads();
    }
    if (tid == 0) {
        b.stats[0] += n_map; b.stats[1] += n_ckpt; b.stats[2] += n_serial; b.stats[3] = (int32_t)stop_at;
        *b.resume = T;
        // the shard's end state: the carrying candidate's, else T (the last chunk ran serially, or is fully gated)
        if constexpr (SH) b.resume[1] = (cand >= 0) ? b.E[(n_chunks - 1) * K + cand] : T;
        if constexpr (DEV) {
            CostasCtl *ctl = costas_ctl(b);
            if (stop_at < n_chunks) { ctl->c_from = stop_at; ctl->use_seed = 1; ctl->seed_freq = T.freq; ctl->rounds += 1; }
            else ctl->done = 1;
            b.stats[4] = ctl->rounds;
        }
    }
}

// Output pass: every chunk from its TRUE start state.  A chunk that lies on a candidate's trajectory from its first
// sample (gidx >= 0) is evaluated by kNumCkpt lanes, each from the candidate's checkpoint state (bitwise the true state
// there); any other chunk by one lane from T[c].
template <int DT, int ORDER, bool SH = false>
__global__ __launch_bounds__(256) void k_costas_final(const CostasArgsT<SH> a_in, SpecBuffers b, int64_t n_chunks, int K) {
    const CostasArgsT<SH> a = costas_device_noise(a_in);
    const int64_t gid = blockIdx.x * 256ll + threadIdx.x;
    const int64_t c = gid / kNumCkpt;
    const int j = (int)(gid % kNumCkpt);            // segment j = samples [j kCkpt, (j + 1) kCkpt) of the chunk
    if (c >= n_chunks) return;
    if (gid == 0 && a.n > 0 && chunk0_exact<SH>(a)) a.out[0] = -4.0f;      // reference: np.empty, never written (documented in urhgpu.h)
    const int64_t s0 = chunk_begin_of<SH>(a, c);
    const int64_t e0 = (s0 + kChunk < a.n) ? s0 + kChunk : a.n;
    const int g = b.gidx[c];
    int64_t i0 = s0, i1 = e0;
    CostasState st = b.T[c];
    if (g >= 0) {
        i0 = s0 + (int64_t)j * kCkpt;
        i1 = (i0 + kCkpt < e0) ? i0 + kCkpt : e0;
        if (j > 0) st = b.CP[(c * kNumCkpt + (j - 1)) * K + g];
    } else if (j != 0) return;
    float err = 0.0f;
    // 16 samples (one 128-byte line of complex64) per round: the lanes of a wavefront are 2 KiB apart, so every line a lane
    // touches is fetched for that lane alone -- ask for all of it at once instead of 16 times 8 bytes
    constexpr int kTileF = 16;
    int64_t i = i0;
    for (; i + kTileF <= i1; i += kTileF) {
        float2 x[kTileF];
#pragma unroll
        for (int u = 0; u < kTileF; ++u) x[u] = CostasLoad<DT>::at(a.iq, i + u);
        float o[kTileF];
#pragma unroll 1
        for (int u = 0; u < kTileF; ++u) {
            float2 xv = x[0];
#pragma unroll
            for (int q = 1; q < kTileF; ++q) if (u == q) xv = x[q];
            const float ov = costas_step_bf<DT == URHGPU_DT_F32, ORDER>(xv, st, err, a);
#pragma unroll
            for (int q = 0; q < kTileF; ++q) if (u == q) o[q] = ov;
        }
#pragma unroll
        for (int u = 0; u < kTileF; ++u) a.out[i + u] = o[u];
    }
    for (; i < i1; ++i) a.out[i] = costas_step_bf<DT == URHGPU_DT_F32, ORDER>(CostasLoad<DT>::at(a.iq, i), st, err, a);
}

constexpr size_t kCtlSlot = 64;    // the control block's place behind the stats (spec_buffers)
static_assert(sizeof(CostasCtl) <= kCtlSlot, "control block");
size_t costas_scratch_bytes(int64_t n) {
    const int64_t nc = (std::max<int64_t>(n - 1, 0) + kChunk - 1) / kChunk + 1;
    return (size_t)nc * kMaxCand * sizeof(CostasState) * 2 + (size_t)nc * kNumCkpt * kMaxCand * sizeof(CostasState) +
           (size_t)nc * 4 * 3 + (size_t)nc * sizeof(CostasState) + (size_t)nc * kMaxCand * 5 + 3 * 64 + kCtlSlot + 16 * 256;
}

constexpr int kMaxRounds = 24;     // re-speculation rounds before the stitch stops handing back (and runs serially)
std::atomic<long long> g_costas_host_syncs{0};     // urhgpu_test_costas_host_syncs: hipStreamSynchronize calls of the host-driven loops

// the speculative buffers of nc chunks, carved from costas_scratch_bytes(n) of scratch
static SpecBuffers spec_buffers(void *scratch, int64_t nc, int K) {
    char *p = (char *)scratch;
    auto take = [&](size_t bytes) { char *r = p; p += (bytes + 255) & ~size_t(255); return r; };
    SpecBuffers b;
    b.S = (CostasState *)take((size_t)nc * K * sizeof(CostasState));
    b.E = (CostasState *)take((size_t)nc * K * sizeof(CostasState));
    b.CP = (CostasState *)take((size_t)nc * kNumCkpt * K * sizeof(CostasState));
    b.map = (uint32_t *)take((size_t)nc * 4);
    b.T = (CostasState *)take((size_t)nc * sizeof(CostasState));
    b.ungated = (int32_t *)take((size_t)nc * 4);
    b.gidx = (int32_t *)take((size_t)nc * 4);
    b.run_list = (int32_t *)take((size_t)nc * K * 4);
    b.is_rep = (uint8_t *)take((size_t)nc * K);
    b.run_count = (int32_t *)take(64);
    b.resume = (CostasState *)take(64);
    b.stats = (int32_t *)take(64 + kCtlSlot);           // stats and control block: zeroed by one memset
    return b;
}
// (test hook) scratch bytes reserved for n samples / one past the control block as spec_buffers carves it / the block's size
void costas_scratch_layout(int64_t n, int K, int64_t out3[3]) {
    const int64_t nc = (std::max<int64_t>(n - 1, 0) + kChunk - 1) / kChunk;
    const SpecBuffers b = spec_buffers(nullptr, nc, K);
    out3[0] = (int64_t)costas_scratch_bytes(n);
    out3[1] = (int64_t)(uintptr_t)costas_ctl(b) + (int64_t)sizeof(CostasCtl);
    out3[2] = (int64_t)sizeof(CostasCtl);
}

// NOTE: synchronises the stream (at least once): the host has to learn whether the chunk chain closed.
template <int DT, int ORDER>
static int launch_costas_spec(const CostasArgs &a, void *scratch, urhgpu_ctx *ctx);
// ... and the same rounds driven from the device: nothing but launches and one asynchronous copy of the stats.
template <int DT, int ORDER>
static int launch_costas_dev(const CostasArgs &a, void *scratch, urhgpu_ctx *ctx, int rounds, int32_t *h_stats);

// Re-speculation rounds the device-driven loop queues for a capture of nc chunks when nobody says (tuning key costas_dev_rounds = -1).
// A round that finds the chain closed is a 4-byte memset and four launches that return on one load: kEmptyRoundUs.  Too few rounds have a
// cliff -- behind the last one the rest of the capture is walked by one wavefront, 1.5 ms per chunk --, so the rule spends what is cheap: as
// many rounds as fit into kEmptyRoundsShare of the pass's own Costas time, kCostasBaseUs (the latency of one chunk's candidate, run and
// output pass: what the shortest parallel capture already pays) plus kCostasUsPerChunk for every chunk; never fewer than 2, never more
// than the host loop's 24.  That is 7 rounds for the shortest parallel capture and 13 for 2^27 samples.
// NOT MEASURED YET: the three figures are estimates -- five stream packets at about 5 us each; (512 warm-up + 4096 + 256) steps of 94
// dependent instructions at 9.5 cycles and 2.4 GHz (the step anatomy above costas_step_bf); the 3.3 ms Costas time of 32 768 chunks
// (profiles/r04f_costas_1gib_kernel_stats.csv).  tools/psk_stream_probe.py measures all three ((c), and (c)'s 0-round times over the
// sizes); replace them by its figures.
constexpr double kEmptyRoundUs = 25.0, kCostasBaseUs = 1800.0, kCostasUsPerChunk = 0.046, kEmptyRoundsShare = 0.10;
static int costas_auto_rounds(int64_t nc) {
    const double fit = kEmptyRoundsShare * (kCostasBaseUs + kCostasUsPerChunk * (double)nc) / kEmptyRoundUs;
    return (int)std::min<double>(kMaxRounds, std::max<double>(2.0, fit));
}

// Which loop: the host-driven one for one-shot passes on a context that is not pipelined; the device-driven one on pipelined contexts
// (capture streams switch theirs) and wherever the tuning key costas_dev_rounds names a number of rounds.
// The stats land in ctx->costas_stats_next where a capture stream has named a place of its pass's own, else in h_counts[12..].
template <int DT>
static int launch_costas_dt(const CostasArgs &a, void *scratch, urhgpu_ctx *ctx) {
    const bool parallel = (a.loop_order == 2 || a.loop_order == 4) && a.n > 2 * kChunk && scratch != nullptr;
    int32_t *h_stats = ctx->costas_stats_next ? ctx->costas_stats_next : (int32_t *)(ctx->h_counts + 12);
    if (!parallel) {
        hipLaunchKernelGGL(k_costas<DT>, dim3(1), dim3(64), 0, ctx->stream, a);
        memset(h_stats, 0, 24);
        return URHGPU_OK;
    }
    if (ctx->tune_costas_dev_rounds >= 0 || ctx->pipelined) {
        const int rounds = ctx->tune_costas_dev_rounds >= 0 ? ctx->tune_costas_dev_rounds : costas_auto_rounds((a.n - 1 + kChunk - 1) / kChunk);
        return dispatch_bool(a.loop_order == 4, [&](auto o4) { return launch_costas_dev<DT, o4.value ? 4 : 2>(a, scratch, ctx, rounds, h_stats); });
    }
    return dispatch_bool(a.loop_order == 4, [&](auto o4) { return launch_costas_spec<DT, o4.value ? 4 : 2>(a, scratch, ctx); });
}

template <int DT, int ORDER>
static int launch_costas_dev(const CostasArgs &a, void *scratch, urhgpu_ctx *ctx, int rounds, int32_t *h_stats) {
    hipStream_t s = ctx->stream;
    const int K = (a.loop_order == 4) ? 8 : 4;
    const int64_t nc = (a.n - 1 + kChunk - 1) / kChunk;
    SpecBuffers b = spec_buffers(scratch, nc, K);
    URH_HIP(hipMemsetAsync(b.stats, 0, 64 + kCtlSlot, s));   // the stats and the control block: round 0 starts at chunk 0, unseeded
    URH_HIP(hipMemsetAsync(b.resume, 0, 64, s));
    // every round's grids cover all nc chunks: where a round starts is known on the device only
    const dim3 g_cand((unsigned)((nc * K + 255) / 256)), g_chunk((unsigned)((nc + 255) / 256));
    for (int round = 0; round <= rounds; ++round) {
        URH_HIP(hipMemsetAsync(b.run_count, 0, 4, s));       // (a round that finds the chain closed appends nothing: k_costas_run sees 0 entries)
        hipLaunchKernelGGL((k_costas_spec<DT, ORDER, false, true>), g_cand, dim3(256), 0, s, a, b, nc, K, (int64_t)0, 0, 0.0f);
        hipLaunchKernelGGL((k_costas_run<DT, ORDER>), g_cand, dim3(256), 0, s, a, b, K);
        hipLaunchKernelGGL(k_costas_map<true>, g_chunk, dim3(256), 0, s, b, nc, K, (int64_t)1);
        hipLaunchKernelGGL((k_costas_stitch<DT, ORDER, false, true>), dim3(1), dim3(kStitchBlock), 0, s, a, b, nc, K, (int64_t)1, round < rounds ? 1 : 0);
    }
    hipLaunchKernelGGL((k_costas_final<DT, ORDER>), dim3((unsigned)((nc * kNumCkpt + 255) / 256)), dim3(256), 0, s, a, b, nc, K);
    URH_HIP(hipGetLastError());
    URH_HIP(hipMemcpyAsync(h_stats, b.stats, 20, hipMemcpyDeviceToHost, s));     // valid once the pass has been synchronised
    return URHGPU_OK;
}

template <int DT, int ORDER>
static int launch_costas_spec(const CostasArgs &a, void *scratch, urhgpu_ctx *ctx) {
    hipStream_t s = ctx->stream;
    const int K = (a.loop_order == 4) ? 8 : 4;
    const int64_t nc = (a.n - 1 + kChunk - 1) / kChunk;
    SpecBuffers b = spec_buffers(scratch, nc, K);
    URH_HIP(hipMemsetAsync(b.stats, 0, 64, s));
    URH_HIP(hipMemsetAsync(b.resume, 0, 64, s));
    int64_t c_from = 0;
    int use_seed = 0;
    float seed_freq = 0.0f;
    int32_t *h = (int32_t *)(ctx->h_counts + 12);            // pinned: stats[0..4], then the resume state
    int rounds = 0;
    for (int round = 0;; ++round) {
        const int64_t todo = nc - c_from;
        URH_HIP(hipMemsetAsync(b.run_count, 0, 4, s));
        hipLaunchKernelGGL((k_costas_spec<DT, ORDER>), dim3((unsigned)((todo * K + 255) / 256)), dim3(256), 0, s, a, b, nc, K, c_from, use_seed,
                           seed_freq);
        hipLaunchKernelGGL((k_costas_run<DT, ORDER>), dim3((unsigned)((todo * K + 255) / 256)), dim3(256), 0, s, a, b, K);
        hipLaunchKernelGGL(k_costas_map<false>, dim3((unsigned)((todo + 255) / 256)), dim3(256), 0, s, b, nc, K, std::max<int64_t>(c_from, 1));
        hipLaunchKernelGGL((k_costas_stitch<DT, ORDER>), dim3(1), dim3(kStitchBlock), 0, s, a, b, nc, K, std::max<int64_t>(c_from, 1),
                           round < kMaxRounds ? 1 : 0);
        URH_HIP(hipGetLastError());
        URH_HIP(hipMemcpyAsync(h, b.stats, 20, hipMemcpyDeviceToHost, s));
        URH_HIP(hipMemcpyAsync(h + 6, b.resume, 8, hipMemcpyDeviceToHost, s));
        URH_HIP(hipStreamSynchronize(s));
        ++g_costas_host_syncs;
        center_note_wait();
        const int64_t stop_at = h[3];
        if (stop_at >= nc) break;
        c_from = stop_at;
        use_seed = 1;
        memcpy(&seed_freq, h + 6, 4);                        // resume state: {freq, phase}
        rounds = round + 1;
    }
    h[4] = rounds;
    hipLaunchKernelGGL((k_costas_final<DT, ORDER>), dim3((unsigned)((nc * kNumCkpt + 255) / 256)), dim3(256), 0, s, a, b, nc, K);
    return URHGPU_OK;
}

int launch_costas(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad, void *scratch, const float *d_noise) {
    CostasArgs a;
    a.iq = d_iq; a.n = n; a.out = d_qad; a.d_noise = d_noise;
    URH_TRY(costas_args(p, a));
    return dispatch_dtype(p->dtype, [&](auto dt) { return launch_costas_dt<dt.value>(a, scratch, ctx); });      // (costas_args has refused every other code)
}

// ---- sharded captures: one rank's Costas pass (include/urhgpu.h, "PSK across shards") ----------------------------------------
// A shard is the single-GPU problem one level up: its chunk 0 is a chunk whose true start state lives on another GPU.  The rank
// speculates its chunks (SH instantiations: chunks from the shard's start, walks back into the raw left halo), reduces them to a
// fixed-size summary, and -- once the ranks have composed the summaries into its true start state -- stitches from that state and
// runs the output pass.

int64_t costas_halo_samples(const urhgpu_params *p) { return (int64_t)kWarmBackFactor * costas_warm(p->costas_loop_bandwidth); }

// The summary (kCostasSummaryBytes, uint32 words): what the other ranks need to carry the loop state across the shard without its
// samples.  One workgroup; the chunk maps are composed as in the stitch's fast-forward (map_compose, wave scan), reduced to their total.
//   0 .. 15   start states {freq, phase} of chunk 0's candidates (float32 bits; candidates >= K: 0)
//   16 .. 31  end states of the last chunk's candidates (representatives only, others 0)
//   32        map[n_chunks - 1] o ... o map[1]: chunk-0 candidate -> last-chunk candidate carrying the same trajectory, 0xF = broken
//   33        bit k: chunk 0's candidate k is a representative (no lower-numbered candidate starts in the same state)
//   34        1: no un-gated sample in the shard (gated samples freeze the loop: end state = start state)
//   35        K;  36 .. 37: n_chunks (int64);  38 .. 39: un-gated samples (int64)
constexpr int kSumBlock = 1024;
__global__ __launch_bounds__(kSumBlock) void k_costas_shard_summary(SpecBuffers b, int64_t n_chunks, int K, uint32_t *out) {
    __shared__ uint32_t s_wp[kSumBlock / 64];
    __shared__ unsigned long long s_ung;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_ung = 0;
    __syncthreads();
    unsigned long long ung = 0;
    for (int64_t c = tid; c < n_chunks; c += kSumBlock) ung += (uint32_t)b.ungated[c];
    atomicAdd(&s_ung, ung);
    uint32_t R = 0x76543210u;                                   // composition of the maps so far (every thread keeps it)
    constexpr int Q = 4;
    for (int64_t c0 = 1; c0 < n_chunks; c0 += (int64_t)kSumBlock * Q) {
        const int64_t cc0 = c0 + (int64_t)Q * tid;
        uint32_t P = 0x76543210u;
#pragma unroll
        for (int q = 0; q < Q; ++q) if (cc0 + q < n_chunks) P = map_compose(b.map[cc0 + q], P);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                      // lane 63: the wavefront's chunks in order
            const uint32_t u = __shfl_up(P, o);
            if (lane >= o) P = map_compose(P, u);
        }
        if (lane == 63) s_wp[wave] = P;
        __syncthreads();
        for (int w = 0; w < kSumBlock / 64; ++w) R = map_compose(s_wp[w], R);
        __syncthreads();
    }
    __syncthreads();
    if (tid < kCostasSummaryBytes / 4) {
        const int64_t last = (n_chunks - 1) * K;
        uint32_t v = 0;
        if (tid < 16) {
            const int k = tid >> 1;
            if (k < K) { const CostasState s = b.S[k]; v = __float_as_uint((tid & 1) ? s.phase : s.freq); }
        } else if (tid < 32) {
            const int k = (tid - 16) >> 1;
            if (k < K && b.is_rep[last + k]) { const CostasState e = b.E[last + k]; v = __float_as_uint((tid & 1) ? e.phase : e.freq); }
        } else if (tid == 32) {
            v = R;
        } else if (tid == 33) {
            for (int k = 0; k < K; ++k) v |= b.is_rep[k] ? (1u << k) : 0u;
        } else if (tid == 34) {
            v = (s_ung == 0) ? 1u : 0u;
        } else if (tid == 35) {
            v = (uint32_t)K;
        } else if (tid < 38) {
            v = (uint32_t)((uint64_t)n_chunks >> (32 * (tid - 36)));
        } else {
            v = (uint32_t)(s_ung >> (32 * (tid - 38)));
        }
        out[tid] = v;
    }
}

__global__ void k_costas_set_state(CostasState *dst, uint32_t freq_bits, uint32_t phase_bits) {     // bits as given (NaN payloads too)
    uint32_t *d = (uint32_t *)dst;
    d[0] = freq_bits; d[1] = phase_bits;
}

static int costas_shard_args(const CostasShard &cs, CostasArgsSh &a, int64_t &nc) {
    a.iq = cs.iq; a.n = cs.n; a.out = cs.out;
    URH_TRY(costas_args(&cs.p, a));
    if (a.loop_order != 2 && a.loop_order != 4) return URHGPU_ERR_UNSUPPORTED;    // the reference leaves the output unwritten
    a.halo_end = cs.halo_end; a.origin = cs.origin; a.lo = cs.lo; a.start1 = cs.start1;
    nc = (cs.n - cs.origin + kChunk - 1) / kChunk;
    return URHGPU_OK;
}

template <int DT, int ORDER>
static int costas_shard_spec_t(urhgpu_ctx *ctx, const CostasArgsSh &a, int64_t nc, void *scratch, void *d_summary) {
    hipStream_t s = ctx->stream;
    const int K = (ORDER == 4) ? 8 : 4;
    const SpecBuffers b = spec_buffers(scratch, nc, K);
    URH_HIP(hipMemsetAsync(b.stats, 0, 64, s));
    URH_HIP(hipMemsetAsync(b.resume, 0, 64, s));
    URH_HIP(hipMemsetAsync(b.run_count, 0, 4, s));
    const unsigned g = (unsigned)((nc * K + 255) / 256);
    hipLaunchKernelGGL((k_costas_spec<DT, ORDER, true>), dim3(g), dim3(256), 0, s, a, b, nc, K, (int64_t)0, 0, 0.0f);
    hipLaunchKernelGGL((k_costas_run<DT, ORDER, true>), dim3(g), dim3(256), 0, s, a, b, K);
    hipLaunchKernelGGL(k_costas_map<false>, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, b, nc, K, (int64_t)1);
    hipLaunchKernelGGL(k_costas_shard_summary, dim3(1), dim3(kSumBlock), 0, s, b, nc, K, (uint32_t *)d_summary);
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

// NOTE: synchronises the stream once per stitch round (as launch_costas_spec: the host learns whether the chunk chain closed).
template <int DT, int ORDER>
static int costas_shard_resolve_t(urhgpu_ctx *ctx, const CostasArgsSh &a, int64_t nc, void *scratch, uint32_t freq_bits, uint32_t phase_bits,
                                  void *d_end) {
    hipStream_t s = ctx->stream;
    const int K = (ORDER == 4) ? 8 : 4;
    const SpecBuffers b = spec_buffers(scratch, nc, K);
    hipLaunchKernelGGL(k_costas_set_state, dim3(1), dim3(1), 0, s, b.resume, freq_bits, phase_bits);
    int64_t c_from = 0;
    float seed_freq = 0.0f;
    int32_t *h = (int32_t *)(ctx->h_counts + 12);            // pinned: stats[0..4], then the resume state
    int rounds = 0;
    for (int round = 0;; ++round) {
        if (round > 0) {                                     // the chain broke for good inside the shard: re-speculate the rest
            const int64_t todo = nc - c_from;
            URH_HIP(hipMemsetAsync(b.run_count, 0, 4, s));
            hipLaunchKernelGGL((k_costas_spec<DT, ORDER, true>), dim3((unsigned)((todo * K + 255) / 256)), dim3(256), 0, s, a, b, nc, K, c_from, 1,
                               seed_freq);
            hipLaunchKernelGGL((k_costas_run<DT, ORDER, true>), dim3((unsigned)((todo * K + 255) / 256)), dim3(256), 0, s, a, b, K);
            hipLaunchKernelGGL(k_costas_map<false>, dim3((unsigned)((todo + 255) / 256)), dim3(256), 0, s, b, nc, K, c_from);
        }
        hipLaunchKernelGGL((k_costas_stitch<DT, ORDER, true>), dim3(1), dim3(kStitchBlock), 0, s, a, b, nc, K, c_from,
                           round < kMaxRounds ? 1 : 0);
        URH_HIP(hipGetLastError());
        URH_HIP(hipMemcpyAsync(h, b.stats, 20, hipMemcpyDeviceToHost, s));
        URH_HIP(hipMemcpyAsync(h + 6, b.resume, 8, hipMemcpyDeviceToHost, s));
        URH_HIP(hipStreamSynchronize(s));
        ++g_costas_host_syncs;
        center_note_wait();
        const int64_t stop_at = h[3];
        if (stop_at >= nc) break;
        c_from = stop_at;                                    // >= 1: the stitch stops in front of the chunk after the one it ran
        memcpy(&seed_freq, h + 6, 4);
        rounds = round + 1;
    }
    h[4] = rounds;
    if (d_end) URH_HIP(hipMemcpyAsync(d_end, b.resume + 1, 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL((k_costas_final<DT, ORDER, true>), dim3((unsigned)((nc * kNumCkpt + 255) / 256)), dim3(256), 0, s, a, b, nc, K);
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int launch_costas_shard_spec(urhgpu_ctx *ctx, const CostasShard &cs, void *d_summary) {
    CostasArgsSh a;
    int64_t nc = 0;
    URH_TRY(costas_shard_args(cs, a, nc));
    return dispatch_dtype(cs.p.dtype, [&](auto dt) {
        return dispatch_bool(a.loop_order == 4, [&](auto o4) { return costas_shard_spec_t<dt.value, o4.value ? 4 : 2>(ctx, a, nc, cs.scratch, d_summary); });
    });
}

int launch_costas_shard_resolve(urhgpu_ctx *ctx, const CostasShard &cs, uint32_t freq_bits, uint32_t phase_bits, void *d_end) {
    CostasArgsSh a;
    int64_t nc = 0;
    URH_TRY(costas_shard_args(cs, a, nc));
    return dispatch_dtype(cs.p.dtype, [&](auto dt) {
        return dispatch_bool(a.loop_order == 4, [&](auto o4) {
            return costas_shard_resolve_t<dt.value, o4.value ? 4 : 2>(ctx, a, nc, cs.scratch, freq_bits, phase_bits, d_end);
        });
    });
}

// every float with |y| < 120 (bit patterns 0 .. 0x42f00000, both signs): urh_sincosf_fast against urh_sinf / urh_cosf
__global__ __launch_bounds__(256) void k_test_sincosf_fast(unsigned long long *mismatches) {
    unsigned long long bad = 0;
    for (uint64_t u = blockIdx.x * 256ull + threadIdx.x; u < 2ull * 0x42f00000ull; u += (uint64_t)gridDim.x * 256ull) {
        const uint32_t bits = (u < 0x42f00000ull) ? (uint32_t)u : ((uint32_t)(u - 0x42f00000ull) | 0x80000000u);
        const float y = __uint_as_float(bits);
        float sn, cs;
        urh_sincosf_fast(y, &sn, &cs);
        if (__float_as_uint(sn) != __float_as_uint(urh_sinf(y)) || __float_as_uint(cs) != __float_as_uint(urh_cosf(y))) ++bad;
    }
    if (bad) atomicAdd(mismatches, bad);
}
void launch_test_sincosf_fast(unsigned long long *d_mismatches, hipStream_t s) {
    hipLaunchKernelGGL(k_test_sincosf_fast, dim3(256 * 32), dim3(256), 0, s, d_mismatches);
}

}  // namespace urh
