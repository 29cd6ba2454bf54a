// batch_kernels.hpp -- the walk of a batch of captures (batch.hip: a WAVEFRONT PER CAPTURE), shared by the translation units that
// instantiate it: batch.hip (every capture gated with p.noise_sqrd), batch_auto.hip (DNOISE: every capture gated with the threshold
// detected for it, k_batch_noise) and batch_center.hip (QIN: the captures are demodulated already and each is classified through the
// thresholds of its own center).  One definition of k_batch_bits, BatchArgs, batch_region, batch_capture and their helpers, so that the
// routes cannot drift apart.  A translation unit includes this header FIRST: it defines the URH_FDIV / URH_FSQRT forms that the
// headers below it pick up.
#pragma once
#include <hip/hip_runtime.h>

// The quotients and square roots of this file's kernels are taken in fp64 and rounded once to fp32: for fp32 operands that IS the correctly
// rounded fp32 result (53 >= 2 * 24 + 2 bits: the second rounding is innocuous), the float the reference computes -- its ASK branch is even
// written that way, (double)sqrtf / (double)max (:372).  Why: the compiler expands an fp32 division into five v_fma_f32 and a square root
// into two, and without those an fp32 FMA in this file's assembly can only be a contracted multiply-add of the source, which
// tests/test_batch_host.py can then look for.  The empty asm keeps the optimiser from folding the form back into the fp32 division.
__host__ __device__ __forceinline__ float batch_fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    double da = a, db = b;
    __asm__ volatile("" : "+v"(da), "+v"(db));
    return (float)(da / db);
#else
    return a / b;
#endif
}
__host__ __device__ __forceinline__ float batch_fsqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double dx = x;
    __asm__ volatile("" : "+v"(dx));
    return (float)__builtin_sqrt(dx);
#else
    return __builtin_sqrtf(x);
#endif
}
#define URH_FDIV(a, b) batch_fdiv((a), (b))
#define URH_FSQRT(x) batch_fsqrt(x)
#include "common.hpp"
#include "compact.hpp"
#include "demod_prims.hpp"
#include "dispatch.hpp"

namespace urh {

constexpr int kBatchStep = 64;             // samples per step of k_batch_bits: one per lane
constexpr int kBatchCounts = 8;            // int64 per capture: {rows stored, messages, bits, rows needed, truncated, 0, 0, 0}
constexpr int64_t kBatchBadStart = 8;      // truncated bit 3: the capture's start / end are not inside the buffer, or its plan entry is not inside the work buffer

struct BatchArgs {
    const void *iq;            // K captures back to back, (total, 2) of the dtype
    const int64_t *start;      // [k + 1] first sample of each capture
    const int64_t *plan;       // [3 k] region offset (bytes), row capacity, launch order
    int64_t k, total;
    float *qad;                // [total] or nullptr
    char *work;
    int64_t work_bytes;
    int64_t *counts;           // [k][kBatchCounts]
    int64_t *dir;              // [k + 1] blob offsets
    char *blob;
    int64_t cap_blob;
    int64_t pause_threshold;
    uint32_t sps;
    int bps, tol;
    // parameters per capture (batch_each.hip, the EACH forms below; not read elsewhere): the table, the shared thresholds, and the slice of
    // the plan's launch order this walk launch takes
    const urhgpu_batch_each *each;   // [k]
    const float *each_thr;           // [n_thr]
    int64_t n_thr;
    int64_t each_lo, each_n;
};

// a capture's region of the work buffer: what a wavefront may write, from its length and its row capacity alone (host and device agree)
struct BatchRegion { int64_t cap_rows, cap_bits, cap_msg, off_rows, off_bits, off_msg_off, off_pauses, bytes; };
__host__ __device__ inline BatchRegion batch_region(int64_t n, int64_t cap_rows, uint32_t sps, int bps) {
    BatchRegion R;
    auto up = [](int64_t x) { return (x + 15) & ~int64_t(15); };
    R.cap_rows = cap_rows < 0 ? 0 : cap_rows;
    // a message needs a data row and the long pause that closes it; a row of L > 0 samples gives at most L / sps + 1/2 symbols and the
    // positive lengths of a table sum to at most n: neither can overflow while the rows fit
    R.cap_msg = R.cap_rows / 2 + 1;
    R.cap_bits = ((int64_t)((uint32_t)n / sps) + R.cap_rows / 2 + 2) * bps;       // (n < 2^31: a 32-bit quotient)
    int64_t o = 0;
    R.off_rows = o; o = up(o + 8 * R.cap_rows);          // int32 {length, state} per row: one store
    R.off_bits = o; o = up(o + R.cap_bits);
    R.off_msg_off = o; o = up(o + 8 * (R.cap_msg + 1));
    R.off_pauses = o; o = up(o + 8 * R.cap_msg);
    R.bytes = o;
    return R;
}

// what capture c may use: its samples and its region, checked against the buffers (a wavefront never leaves either)
struct BatchCapture { int64_t s0, n, roff; BatchRegion R; bool ok; };
__device__ __forceinline__ BatchCapture batch_capture(const BatchArgs &b, int64_t c, uint32_t sps, int bps, bool each_ok = true) {
    BatchCapture v;
    v.s0 = b.start[c];
    const int64_t s1 = b.start[c + 1];
    v.ok = v.s0 >= 0 && s1 >= v.s0 && s1 <= b.total && s1 - v.s0 <= 0x7fffffffll;
    v.n = v.ok ? s1 - v.s0 : 0;
    v.roff = b.plan[c];
    const int64_t cap_rows = b.plan[b.k + c];
    v.R = batch_region(v.n, v.ok ? cap_rows : 0, sps, bps);
    if (cap_rows < 0 || cap_rows > 0x7fffffffll || v.roff < 0 || (v.roff & 15) || v.roff > b.work_bytes || v.R.bytes > b.work_bytes - v.roff) v.ok = false;
    if (!each_ok) { v.ok = false; v.n = 0; }               // (a record the device does not accept: a refused capture)
    if (!v.ok) {                                           // no region: nothing is stored, everything is still counted
        v.R = batch_region(0, 0, sps, bps);
        v.R.cap_bits = v.R.cap_msg = 0;
    }
    return v;
}
__device__ __forceinline__ BatchCapture batch_capture(const BatchArgs &b, int64_t c) { return batch_capture(b, c, b.sps, b.bps); }

// capture c's record of the per-capture table as the device accepts it: the ranges of batch_check_params, its order - 1 thresholds inside the
// shared table, the noise value of its modulation.  Anything else is a refused capture: the record's values are not followed anywhere.
__device__ __forceinline__ bool batch_each_ok(const urhgpu_batch_each &e, int64_t n_thr) {
    if (e.mod != URHGPU_MOD_ASK && e.mod != URHGPU_MOD_FSK) return false;
    if (e.bits_per_symbol < 1 || e.bits_per_symbol > 7 || e.samples_per_symbol < 1 || e.tolerance < 0 || e.tolerance > 65535) return false;
    if (e.thr_first < 0 || (int64_t)e.thr_first + ((1 << e.bits_per_symbol) - 1) > n_thr) return false;
    return e.noise_val == (e.mod == URHGPU_MOD_ASK ? 0.0f : -4.0f);
}
// ... and capture c's samples and region from ITS samples per symbol and bits per symbol (a refused record: 1 and 1, no region)
__device__ __forceinline__ BatchCapture batch_capture_each(const BatchArgs &b, int64_t c) {
    const urhgpu_batch_each e = b.each[c];
    const bool ok = batch_each_ok(e, b.n_thr);
    return batch_capture(b, c, ok ? e.samples_per_symbol : 1u, ok ? e.bits_per_symbol : 1, ok);
}

__device__ __forceinline__ float batch_shr1(float x, float lane0) {       // value of lane - 1; lane 0 receives `lane0`
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(lane0), __float_as_int(x), 0x138 /*wave_shr:1*/, 0xf, 0xf, false));
}
__device__ __forceinline__ uint32_t batch_shr1(uint32_t x, uint32_t lane0) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)lane0, (int)x, 0x138, 0xf, 0xf, false);
}
// (this clang has no __builtin_amdgcn_writelane; the LLVM intrinsic is reached through its assembler name, as in demod_runs.hip)
extern "C" __device__ int urh_llvm_writelane_i32(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
__device__ __forceinline__ int batch_lane(int x, int lane) { return __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(lane)); }

// classify<ORDER2, true> with the thresholds at `t` instead of p.d_thr (the kernel's argument block cannot be pointed at a capture's own
// thresholds; a copy of it with another d_thr would live in scratch memory): the same text, classify_thr (demod_prims.hpp); t == nullptr: p.thr
template <bool ORDER2>
__device__ __forceinline__ uint32_t classify_at(float q, const RunArgs &p, const float *t, bool check_noise = true) {
    if (check_noise && q == p.noise_val) return kStPause;
    return t ? classify_thr<ORDER2>(q, t, p.order) : classify<ORDER2>(q, p, false);
}

// DNOISE (batch_auto.hip): p.d_noise is the base of the batch's K urhgpu_noise_result blocks (k_batch_noise has written them on the same
// stream) and capture c is gated with ITS block's noise_sqrd, loaded once (a uniform address).  Flag 2 -- the threshold is not below the
// sample type's max_magnitude: the reference demodulates nothing and slices zeros(2) (Signal.py:474-484) -- is walked as a capture of two
// samples, which the n <= 2 rule below turns into two zeros.  Without DNOISE the kernel reads p.noise_sqrd exactly where it always did.
// QIN (batch_center.hip): the captures are ALREADY demodulated -- b.qad is the input, q = qad[s0 + i] as it lies there (k_batch_demod has
// applied the rules of sample 0 and of n <= 2; a caller's own signal is sliced as it is) -- and capture c is classified through ITS order - 1
// thresholds at p.d_thr + c (order - 1) (classify_at, the device-threshold form of classify<ORDER2, true>: k_batch_center_publish has
// written them on the same stream), or through p.thr where p.d_thr is null.  p.d_noise, where not null, still tells a flag-2 capture (two
// samples).  DT is not used.
// EACH (batch_each.hip): capture c is walked with ITS record of the table b.each -- samples per symbol, bits per symbol, tolerance, pause
// threshold -- and classified through ITS order - 1 thresholds at b.each_thr + thr_first (the general form: captures of every order share a
// launch; for order 2 it is the ORDER2 form, value for value); the record, the thresholds and the noise block (always DNOISE) are uniform loads.
// The launch takes the slice [b.each_lo, b.each_lo + b.each_n) of the plan's launch order, the captures of modulation MOD; a record the
// device does not accept, or one of another modulation, is a refused capture.  Without EACH every value is read exactly where it always was.
template <int DT, int MOD, bool ORDER2, bool DNOISE = false, bool QIN = false, bool EACH = false>
__global__ __launch_bounds__(64) void k_batch_bits(const RunArgs p, const BatchArgs b) {
    const int lane = (int)threadIdx.x;
    if ((int64_t)blockIdx.x >= (EACH ? b.each_n : b.k)) return;
    const int64_t c = b.plan[2 * b.k + (EACH ? b.each_lo : 0) + blockIdx.x];            // launch order: longest capture first
    if (c < 0 || c >= b.k) return;
    uint32_t e_sps = 0, e_tol = 0;
    int e_order = 2;
    const float *e_thr = nullptr;
    if (EACH) {
        const urhgpu_batch_each e = b.each[c];                 // (a uniform address)
        if (!batch_each_ok(e, b.n_thr) || e.mod != MOD) {      // refused: the counts say so, nothing is read or stored
            if (lane == 0) {
                int64_t *o = b.counts + kBatchCounts * c;
                o[0] = o[1] = o[2] = o[3] = 0; o[4] = kBatchBadStart; o[5] = o[6] = o[7] = 0;
            }
            return;
        }
        e_sps = e.samples_per_symbol; e_tol = (uint32_t)e.tolerance; e_order = 1 << e.bits_per_symbol;
        e_thr = b.each_thr + e.thr_first;
    }
    const BatchCapture cap = EACH ? batch_capture(b, c, e_sps, 31 - __builtin_clz((unsigned)e_order)) : batch_capture(b, c);
    float nsq = 0.0f;
    bool two = false;
    if (DNOISE) {
        const urhgpu_noise_result *r = (const urhgpu_noise_result *)p.d_noise + c;
        nsq = r->noise_sqrd;
        two = r->flag == 2 && cap.n > 2;
    }
    if (QIN && p.d_noise) two = ((const urhgpu_noise_result *)p.d_noise)[c].flag == 2 && cap.n > 2;
    const float *thr_c = (QIN && p.d_thr) ? p.d_thr + c * (int64_t)(p.order - 1) : nullptr;      // (a uniform address)
    const uint32_t n = two ? 2u : (uint32_t)cap.n;             // < 2^31
    const uint32_t tol = EACH ? e_tol : (uint32_t)b.tol;
    const uint32_t sps1 = EACH ? e_sps : b.sps;               // the ASK short-pause rule's samples per symbol
    const char *iq = (const char *)b.iq + cap.s0 * Iq<DT>::kBytes;
    float *qad = b.qad ? b.qad + cap.s0 : nullptr;
    const float *qin = QIN ? b.qad + cap.s0 : nullptr;
    const uint32_t cap_rows = (uint32_t)cap.R.cap_rows;        // 0 without a region: nothing is stored
    int2 *rows = (int2 *)(b.work + (cap.ok ? cap.roff : 0) + cap.R.off_rows);

    // ---- grab_pulse_lens' variables, wave-uniform.  States are the reference's + 1 (PAUSE = 0, as classify returns them). ----
    uint32_t cur_state = kStPause;        // cur_state
    uint32_t pl = 0;                      // pulse_length: at most n + tol < 2^32 (32-bit scalars: the walk's state stays in registers)
    uint32_t run_state = kStNone;         // state of the last sample seen ...
    uint32_t run_len = 0;                 // ... and for how many consecutive samples: consecutive_pause / state_count[] (only one of them is not 0)
    // cur_index, and the row cur_index - 1, which is still held here because the merge of equal neighbours may add to it.  Touched once per
    // row, not per sample: three lanes of a VECTOR register (0: the row's length -- a table's lengths sum to n - tol --, 1: its state, 2:
    // cur_index), so that the scalar registers go to the per-sample state and the demodulation's nest of branches.
    int row_v = 0;
#define BATCH_ROW_GET(k_) __builtin_amdgcn_readlane(row_v, k_)
#define BATCH_ROW_SET(k_, x_) row_v = urh_llvm_writelane_i32((int)(x_), k_, row_v)
    // (macros, not lambdas: captured by reference these variables were given addresses and ended up in scratch memory)
#define BATCH_STORE_ROW(idx_, st_, len_) \
    do { if ((idx_) < cap_rows && lane == 0) rows[idx_] = make_int2((int)(len_), (int)(st_) - 1); } while (0)
    // a row [state, length]: added to the row before when that has the same state, else appended (:467-474 / :486-493)
#define BATCH_EMIT(st_, len_) \
    do { \
        const uint32_t e_st = (st_), e_n = (uint32_t)BATCH_ROW_GET(2); const int32_t e_len = (int32_t)(len_); \
        if (e_n > 0 && (uint32_t)BATCH_ROW_GET(1) == e_st) { BATCH_ROW_SET(0, BATCH_ROW_GET(0) + e_len); } \
        else { \
            if (e_n > 0) BATCH_STORE_ROW(e_n - 1, BATCH_ROW_GET(1), BATCH_ROW_GET(0)); \
            BATCH_ROW_SET(1, e_st); BATCH_ROW_SET(0, e_len); BATCH_ROW_SET(2, e_n + 1); \
        } \
    } while (0)

    float c_b = 0.0f, d_b = 0.0f;                         // the step before (vector registers; its lane 63 is the seam)
    float c_n = 0.0f, d_n = 0.0f;
    if (QIN) { if ((uint32_t)lane < n) c_n = qin[lane]; }
    else if ((uint32_t)lane < n) Iq<DT>::load1(iq, lane, c_n, d_n);
    for (uint32_t base = 0; base < n; base += kBatchStep) {
        const float cc = c_n, dd = d_n;
        const uint32_t i = base + (uint32_t)lane;
        const bool valid = i < n;
        c_n = d_n = 0.0f;
        if (QIN) { if (i + kBatchStep < n) c_n = qin[i + kBatchStep]; }
        else if (i + kBatchStep < n) Iq<DT>::load1(iq, i + kBatchStep, c_n, d_n);  // the next step's samples are on their way during this one's walk
        const float pc = batch_shr1(cc, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c_b), 63)));
        const float pd = batch_shr1(dd, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d_b), 63)));
        float q;
        if (QIN) q = cc;
        else {
            q = demod_one<MOD, DT, DNOISE>(pc, pd, cc, dd, p, nsq);                       // (every lane: selects below instead of two more levels of branches)
            q = (i == 0) ? p.noise_val : q;                                            // :361 (no predecessor: never the neighbouring capture's sample)
            q = (n <= 2) ? 0.0f : q;                                                   // :335-336
        }
        const uint32_t st = EACH ? ((q == p.noise_val) ? kStPause : classify_thr<false>(q, e_thr, e_order))
                                 : (QIN ? classify_at<ORDER2>(q, p, thr_c) : classify<ORDER2>(q, p));
        if (!QIN && qad && valid) qad[i] = q;
        if (base == 0)      // :421-427: PAUSE when sample 0 is NOISE, else the state of the literal 0.0 (s is still 0 there)
            cur_state = ((uint32_t)batch_lane((int)st, 0) == kStPause) ? kStPause
                        : (EACH ? classify_thr<false>(0.0f, e_thr, e_order) : (QIN ? classify_at<ORDER2>(0.0f, p, thr_c, false) : classify<ORDER2>(0.0f, p, false)));
        const uint32_t before = batch_shr1(st, run_state);
        const uint64_t bm = __builtin_amdgcn_ballot_w64(valid && st != before);    // lanes that start a run
        const int cnt = (int)((n - base < kBatchStep) ? (n - base) : kBatchStep);
        // The step's stretches of equal state, one after the other: L samples of state t, continuing the run counted in run_len when the
        // step begins inside the run the last one ended in.  The reference switches at the sample that makes a run of another state than
        // cur_state LONGER than the tolerance (:452-462), the sample tol + 1 - run_len of the stretch; invariant: a run of another state than
        // cur_state is at most tol long when a stretch ends.
        int pos = 0;
        bool go_on = !(bm & 1ull);
        while (pos < cnt) {
            int nxt;
            if (go_on) {
                nxt = bm ? (int)__builtin_ctzll(bm) : cnt;
            } else {
                const uint64_t rest = (pos < 63) ? (bm >> (pos + 1)) : 0ull;
                nxt = rest ? pos + 1 + (int)__builtin_ctzll(rest) : cnt;
                run_state = (uint32_t)batch_lane((int)st, pos); run_len = 0;
            }
            go_on = false;
            const uint32_t t = run_state;
            const uint32_t L = (uint32_t)(nxt - pos);
            if (t != cur_state && run_len + L > tol) {
                const uint32_t k = tol + 1 - run_len;
                pl += k;
                uint32_t r_st = cur_state;
                const int64_t r_len = (int64_t)pl - (int64_t)tol;
                if (MOD == URHGPU_MOD_ASK && r_st == kStPause && r_len < (int64_t)sps1) r_st = 1u;     // the ASK short-pause rule (:464-465): state 0
                BATCH_EMIT(r_st, r_len);
                pl = tol + (L - k);
                cur_state = t;
            } else {
                pl += L;
            }
            run_len += L;
            pos = nxt;
        }
        c_b = cc; d_b = dd;
    }
    if ((uint32_t)BATCH_ROW_GET(2) < n) BATCH_EMIT(cur_state, (int64_t)pl - (int64_t)tol);      // :485-493: the final row (negative for a capture shorter than the tolerance), n = 1 guarded
    const int64_t rows_needed = (uint32_t)BATCH_ROW_GET(2);
    if (rows_needed > 0) BATCH_STORE_ROW((uint32_t)(rows_needed - 1), BATCH_ROW_GET(1), BATCH_ROW_GET(0));
#undef BATCH_EMIT
#undef BATCH_STORE_ROW
#undef BATCH_ROW_GET
#undef BATCH_ROW_SET

    // (the capture's region once more, behind a barrier the optimiser cannot see through: what only the second half needs -- six more
    // pointers and capacities -- does not occupy scalar registers during the first)
    uint32_t wg = blockIdx.x;
    __asm__ volatile("" : "+s"(wg));
    const int64_t c_again = b.plan[2 * b.k + (EACH ? b.each_lo : 0) + wg];
    uint32_t sps = b.sps;
    int bps = b.bps;
    int64_t pt = b.pause_threshold;
    if (EACH) {                                            // (accepted above: the same record once more)
        const urhgpu_batch_each e2 = b.each[c_again];
        sps = e2.samples_per_symbol; bps = e2.bits_per_symbol; pt = e2.pause_threshold;
    }
    const BatchCapture cap2 = EACH ? batch_capture(b, c_again, sps, bps) : batch_capture(b, c_again);
    const BatchRegion R = cap2.R;
    const bool ok = cap2.ok;
    char *region = b.work + (ok ? cap2.roff : 0);
    uint8_t *bits = (uint8_t *)(region + R.off_bits);
    int64_t *msg_off = (int64_t *)(region + R.off_msg_off), *pauses = (int64_t *)(region + R.off_pauses);
    const int64_t nr = rows_needed < R.cap_rows ? rows_needed : R.cap_rows;      // rows that were stored
    const int2 *rows2 = (const int2 *)(region + R.off_rows);

    // ---- _ppseq_to_bits over the stored rows: 64 rows per load, walked one by one; the lanes expand a row's symbols ----
    __syncthreads();                                       // (one wavefront: lane 0's row stores are visible to every lane's loads)
    int64_t nbits = 0, nmsg = 0, msg_bits_start = 0;
    bool there_was_data = false;
    int last_state = 0;
    int64_t last_len = 0;
    if (ok && lane == 0) msg_off[0] = 0;
    for (int64_t rb = 0; rb < nr; rb += 64) {
        int len_v = 0, st_v = 0, nsym_v = 0;
        if (rb + lane < nr) {
            const int2 row = rows2[rb + lane];
            len_v = row.x; st_v = row.y;
            // int(L / sps) + (fraction > 0.5): exact in integers for |L| < 2^31; a negative length truncates towards zero and rounds nowhere
            const uint32_t a = (uint32_t)(len_v < 0 ? -(int64_t)len_v : (int64_t)len_v), qq = a / sps, rr = a - qq * sps;
            nsym_v = len_v < 0 ? -(int)qq : (int)(qq + ((2 * (uint64_t)rr > (uint64_t)sps) ? 1u : 0u));
        }
        const int m = (int)((nr - rb < 64) ? (nr - rb) : 64);
        for (int j = 0; j < m; ++j) {
            const int64_t L = batch_lane(len_v, j), nsym = batch_lane(nsym_v, j);
            const int s = batch_lane(st_v, j);
            last_state = s; last_len = L;
            if (rb + j == 0 && s == -1) continue;          // "starts with pause": only seeds total_samples (:338-340)
            const int64_t k_bits = nsym * bps;
            if (s == -1 && !(nsym <= pt || pt == 0)) {     // a long pause
                if (!there_was_data) {
                    nbits = msg_bits_start;                // drops what was gathered
                } else {
                    if (ok && nmsg < R.cap_msg && lane == 0) { pauses[nmsg] = L; msg_off[nmsg + 1] = nbits; }
                    ++nmsg;
                    msg_bits_start = nbits;
                    there_was_data = false;
                }
                continue;
            }
            if (k_bits > 0) {
                for (int64_t u = lane; u < nsym; u += 64)                          // a symbol per lane: util.number_to_bits, MSB first
                    for (int bb = 0; bb < bps; ++bb) {
                        const int64_t at = nbits + u * bps + bb;
                        if (ok && at < R.cap_bits) bits[at] = (s == -1) ? (uint8_t)0 : (uint8_t)((s >> (bps - 1 - bb)) & 1);
                    }
                nbits += k_bits;
            }
            if (s != -1 && !there_was_data && nsym > 0) there_was_data = true;
        }
    }
    if (there_was_data) {
        if (ok && nmsg < R.cap_msg && lane == 0) { pauses[nmsg] = (last_state == -1) ? last_len : 0; msg_off[nmsg + 1] = nbits; }
        ++nmsg;
    } else {
        nbits = msg_bits_start;                            // bits behind the last message that closed belong to none
    }
    if (lane == 0) {
        int64_t *o = b.counts + kBatchCounts * c_again;
        o[0] = nr;
        o[1] = nmsg < R.cap_msg ? nmsg : R.cap_msg;
        o[2] = nbits < R.cap_bits ? nbits : R.cap_bits;
        o[3] = rows_needed;
        o[4] = ((rows_needed > R.cap_rows || nmsg > R.cap_msg || nbits > R.cap_bits) ? 1 : 0) | (ok ? 0 : kBatchBadStart);
        o[5] = o[6] = o[7] = 0;
    }
}

__device__ __forceinline__ BlobLayout batch_blob_layout(const int64_t *cnt) {
    const int64_t c5[5] = {cnt[0], cnt[1], cnt[2], 0, cnt[3]};
    return blob_layout(c5, cnt[0], cnt[2], cnt[1], 0, 0);
}

// capture c's results as a standard compact blob at dir[c]: header flags 0, int8 states, int32 lengths, bits packed MSB first, no positions
// (EACH, batch_each.hip: the region laid out from the capture's own record)
template <bool EACH>
__global__ __launch_bounds__(64) void k_batch_pack(const BatchArgs b) {
    const int lane = (int)threadIdx.x;
    const int64_t c = blockIdx.x;
    if (c >= b.k) return;
    const int64_t *cnt = b.counts + kBatchCounts * c;
    const BlobLayout L = batch_blob_layout(cnt);
    const int64_t at = b.dir[c];
    if (at < 0 || at > b.cap_blob || L.total > b.cap_blob - at) return;        // (cannot happen with the planned capacity; the fetch reports it)
    const BatchCapture cap = EACH ? batch_capture_each(b, c) : batch_capture(b, c);
    const BatchRegion R = cap.R;
    // (counts that are not this capture's -- a plan whose launch order left it out -- are not followed into the region)
    if (cnt[0] < 0 || cnt[0] > R.cap_rows || cnt[1] < 0 || cnt[1] > R.cap_msg || cnt[2] < 0 || cnt[2] > R.cap_bits) return;
    char *out = b.blob + at;
    // (EACH: a capture the walk refused -- a record of another modulation than its launch's -- has a region nothing was written to)
    const bool ok = EACH ? (cap.ok && !(cnt[4] & kBatchBadStart)) : cap.ok;
    const char *region = b.work + (ok ? cap.roff : 0);
    if (lane < 16) {
        int64_t v = 0;
        switch (lane) {
            case 0: v = URHGPU_BLOB_MAGIC; break;
            case 1: v = L.n_rows; break;
            case 2: v = L.n_msg; break;
            case 3: v = L.n_bits; break;
            case 5: v = cnt[3]; break;
            case 6: v = L.total; break;
            case 8: v = L.off_pauses; break;
            case 9: v = L.off_msg_off; break;
            case 10: v = L.off_pos_off; break;
            case 11: v = L.off_row_state; break;
            case 12: v = L.off_bits; break;
            case 13: v = L.off_row_len; break;
            case 14: v = L.off_pos32; break;
            case 15: v = cnt[4]; break;
            default: break;                                 // n_pos, flags: 0
        }
        ((int64_t *)out)[lane] = v;
    }
    if (!ok) {                                              // nothing was stored: the counts are all 0 but msg_off / pos_off [0]
        if (lane == 0) { *(int64_t *)(out + L.off_msg_off) = 0; *(int64_t *)(out + L.off_pos_off) = 0; }
        return;
    }
    const int64_t *pauses = (const int64_t *)(region + R.off_pauses), *msg_off = (const int64_t *)(region + R.off_msg_off);
    int64_t *o_pa = (int64_t *)(out + L.off_pauses), *o_mo = (int64_t *)(out + L.off_msg_off), *o_po = (int64_t *)(out + L.off_pos_off);
    for (int64_t i = lane; i <= L.n_msg; i += 64) {
        if (i < L.n_msg) o_pa[i] = pauses[i];
        o_mo[i] = msg_off[i]; o_po[i] = 0;                  // (positions are derived from the rows on the host)
    }
    const int2 *rows = (const int2 *)(region + R.off_rows);
    int8_t *o_st = (int8_t *)(out + L.off_row_state);
    int32_t *o_len = (int32_t *)(out + L.off_row_len);
    for (int64_t i = lane; i < L.n_rows; i += 64) { const int2 r = rows[i]; o_st[i] = (int8_t)r.y; o_len[i] = r.x; }
    // bits: eight bytes in, one byte out; the bits beyond n_bits of the last byte are zero
    const uint8_t *bits = (const uint8_t *)(region + R.off_bits);
    const unsigned long long *in = (const unsigned long long *)bits;
    uint8_t *o_bits = (uint8_t *)(out + L.off_bits);
    const int64_t nb = (L.n_bits + 7) / 8;
    for (int64_t j = lane; j < nb; j += 64) {
        unsigned long long w;
        if (8 * j + 8 <= L.n_bits) w = in[j];
        else { w = 0; for (int k = 0; k < 8 && 8 * j + k < L.n_bits; ++k) w |= (unsigned long long)bits[8 * j + k] << (8 * k); }
        o_bits[j] = (uint8_t)(((w & 0x0101010101010101ull) * 0x8040201008040201ull) >> 56);
    }
}

// ---- host side, defined in batch.hip and shared with batch_auto.hip ----
// the parameters a batch accepts (every entry point): ASK / FSK, the ranges of the other passes
int batch_check_params(const urhgpu_params *p);
// ... and the PSK entry points': the same ranges, PSK alone
int batch_check_params_psk(const urhgpu_params *p);
// the demodulation's argument block from the parameters of a batch (p has passed batch_check_params)
void batch_run_args(const urhgpu_params *p, RunArgs &a);
// the argument checks of urhgpu_iq_to_bits_batch_dev and the two argument blocks of its launches
int batch_setup(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k, const urhgpu_params *p,
                float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob, RunArgs &a, BatchArgs &b);
// k_batch_scan and k_batch_pack behind a launch of k_batch_bits: two launches
void launch_batch_scan_pack(const BatchArgs &b, unsigned grid, hipStream_t s);
// k_batch_scan alone (batch_each.hip packs with a kernel of its own): one launch
void launch_batch_scan(const BatchArgs &b, hipStream_t s);

// ---- host side, defined in batch_psk.hip and used by batch_center.hip's whole PSK pass ----
// PSK parameters a batch accepts: batch_check_params_psk's, and a loop order the reference writes an output for (2 or 4)
int batch_costas_check(const urhgpu_params *p);
// k_batch_costas: the Costas loop of every capture of b into b.qad, a lane per capture -- ONE launch.  d_noise: nullptr, or the batch's K result blocks
int launch_batch_costas(const urhgpu_params *p, const BatchArgs &b, const urhgpu_noise_result *d_noise, hipStream_t s);

}  // namespace urh
