// batch_records_kernels.hpp -- the kernels behind a batch's walk that make one record per message (batch_records.hip has the account), shared
// by the translation units that instantiate them: batch_records.hip (one parameter set for all captures) and batch_each.hip (EACH: every
// capture with its own record of the per-capture table).  batch_kernels.hpp comes first (its rule).
#pragma once
#include "batch_kernels.hpp"

#include "rec_sum.hpp"

namespace urh {

struct BatchRecArgs {
    BatchArgs b;                 // the walk's block: iq, start (of k_all captures), plan, k, total, work, counts, sps, bps, pause_threshold
    int64_t k_all;               // captures d_start describes (k without a map)
    const int64_t *map;          // nullptr, or [k]: capture j's samples are capture map[j]'s of b.start
    int64_t *rec_dir;            // [k + 1]
    urhgpu_msg_record *rec;
    int32_t *rec_capture;        // [cap_rec] the capture (of b.start) a record's samples lie in
    int64_t cap_rec;
    int64_t divisor;             // <= 1: no padding
    double norm;
};

// the stored messages of capture c as every kernel here counts them: the walk's count, never more than its row capacity allows
__device__ __forceinline__ int64_t rec_msgs(const BatchRecArgs &a, int64_t c) {
    const int64_t n = a.b.counts[kBatchCounts * c + 1], rows = a.b.plan[a.b.k + c];
    const int64_t cap = (rows < 0 || rows > 0x7fffffffll) ? 0 : rows / 2 + 1;
    return n < 0 ? 0 : (n < cap ? n : cap);
}

// capture c's samples and its region as the walk derived them (batch_capture), the samples taken through the map
struct RecCapture { int64_t src, s0, n, roff; BatchRegion R; bool ok; };
__device__ __forceinline__ bool rec_samples(const BatchRecArgs &a, int64_t src, int64_t *s0, int64_t *n) {
    if (src < 0 || src >= a.k_all) return false;
    const int64_t lo = a.b.start[src], hi = a.b.start[src + 1];
    if (!(lo >= 0 && hi >= lo && hi <= a.b.total && hi - lo <= 0x7fffffffll)) return false;
    *s0 = lo; *n = hi - lo;
    return true;
}
// (sps, bps: the capture's own; each_ok false: a record of the per-capture table the device does not accept -- nothing is followed)
__device__ __forceinline__ RecCapture rec_capture_of(const BatchRecArgs &a, int64_t c, uint32_t sps, int bps, bool each_ok = true) {
    RecCapture v;
    v.src = a.map ? a.map[c] : c;
    v.s0 = 0; v.n = 0;
    v.ok = rec_samples(a, v.src, &v.s0, &v.n);
    v.roff = a.b.plan[c];
    const int64_t cap_rows = a.b.plan[a.b.k + c];
    v.R = batch_region(v.n, v.ok ? cap_rows : 0, sps, bps);
    if (cap_rows < 0 || cap_rows > 0x7fffffffll || v.roff < 0 || (v.roff & 15) || v.roff > a.b.work_bytes || v.R.bytes > a.b.work_bytes - v.roff) v.ok = false;
    if (!each_ok) v.ok = false;
    return v;
}
__device__ __forceinline__ RecCapture rec_capture_of(const BatchRecArgs &a, int64_t c) { return rec_capture_of(a, c, a.b.sps, a.b.bps); }

__device__ __forceinline__ void rec_store(const BatchRecArgs &a, int64_t at, int64_t first, int64_t mid, int64_t n_pad, int flag, int64_t src) {
    if (at < 0 || at >= a.cap_rec) return;                 // a message beyond the record capacity is not stored
    urhgpu_msg_record r;
    r.rssi = __builtin_nan(""); r.first_pos = first; r.mid_pos = mid; r.n_pad = (int32_t)n_pad; r.flag = flag;
    a.rec[at] = r;
    a.rec_capture[at] = (int32_t)src;
}

// EACH (urhgpu_batch_msg_records_each_dev): capture c's samples per symbol, bits per symbol and pause threshold are those of ITS record of the
// table a.b.each (a uniform load), and the ASK padding applies only where that record is ASK (a.divisor is then the divisor as given)
template <bool EACH>
__global__ __launch_bounds__(64) void k_batch_rec_pos(const BatchRecArgs a) {
    const int lane = (int)threadIdx.x;
    if ((int64_t)blockIdx.x >= a.b.k) return;
    const int64_t c = a.b.plan[2 * a.b.k + blockIdx.x];        // launch order: longest capture first
    if (c < 0 || c >= a.b.k) return;
    uint32_t c_sps = a.b.sps;
    int c_bps = a.b.bps;
    int64_t c_pt = a.b.pause_threshold, c_div = a.divisor;
    bool e_ok = true;
    if (EACH) {
        const urhgpu_batch_each e = a.b.each[c];
        e_ok = batch_each_ok(e, a.b.n_thr);
        c_sps = e_ok ? e.samples_per_symbol : 1u; c_bps = e_ok ? e.bits_per_symbol : 1; c_pt = e.pause_threshold;
        c_div = e.mod == URHGPU_MOD_ASK ? a.divisor : 1;
    }
    const RecCapture cap = EACH ? rec_capture_of(a, c, c_sps, c_bps, e_ok) : rec_capture_of(a, c);
    const int64_t n_msg = rec_msgs(a, c), base = a.rec_dir[c];
    const int64_t *cnt = a.b.counts + kBatchCounts * c;
    const int64_t nr = cnt[0];
    // a capture whose results were truncated or refused: flag 0 for what it stored; nothing of its region is followed
    const bool sweep = cap.ok && !(cnt[4] & (1 | kBatchBadStart)) && nr >= 0 && nr <= cap.R.cap_rows && n_msg <= cap.R.cap_msg;
    int64_t m = 0;                                             // messages closed so far: the record the sweep writes next
    if (sweep) {
        const char *region = a.b.work + cap.roff;
        const int2 *rows = (const int2 *)(region + cap.R.off_rows);
        const int64_t *msg_off = (const int64_t *)(region + cap.R.off_msg_off), *pauses = (const int64_t *)(region + cap.R.off_pauses);
        const int64_t pt = c_pt, sps = c_sps;
        const int64_t spb = (int64_t)(c_sps / (uint32_t)c_bps);          // int(samples_per_symbol / bits_per_symbol)
        int64_t ts = 0;                                        // total_samples in front of the row
        int64_t nb = 0;                                        // bits gathered for message m
        bool there_was_data = false, have_t = false;
        int64_t first = 0, pos_t = 0;                          // positions of the message's bit 0 and bit t
        // message m as the walk stored it, read before its rows: L bits, n_pad zero bits borrowed, k the middle index after the padding,
        // t = min(k, L - 1) the bit whose position the record needs unless the middle lies at or behind the closing pause's start
        int64_t L = -1, n_pad = 0, k = 0, t = 0;
#define REC_LOAD_MSG() \
        do { \
            L = -1; n_pad = 0; k = 0; t = 0; \
            if (m < n_msg) { \
                L = msg_off[m + 1] - msg_off[m]; \
                n_pad = rec_n_pad(L, pauses[m], sps, c_div); \
                k = (L + n_pad) / 2; \
                t = k < L - 1 ? k : L - 1; \
            } \
        } while (0)
        // closed: np = L + 2 entries, entry L = A, the closing pause's start; trailing: np = L + 1.  k_msg_records: in_pad = n_pad > 0 && k > np - 2,
        // rel = in_pad ? np - 2 : k, mid = pos[rel] + (in_pad ? (k - rel) * sps : 0)
#define REC_CLOSE(closed_, A_) \
        do { \
            const bool c_ok = m < n_msg && L >= 1 && nb == L && have_t; \
            int64_t mid = pos_t; \
            if (closed_) { if (k >= L) mid = (A_) + (k - L) * sps; } \
            else if (k > L - 1) mid = pos_t + (k - (L - 1)) * sps; \
            if (lane == 0 && m < n_msg) rec_store(a, base + m, c_ok ? first : 0, c_ok ? mid : 0, n_pad, c_ok ? 1 : 0, cap.src); \
            ++m; \
        } while (0)
        REC_LOAD_MSG();
        for (int64_t rb = 0; rb < nr; rb += 64) {
            int len_v = 0, st_v = 0, nsym_v = 0;
            if (rb + lane < nr) {
                const int2 row = rows[rb + lane];
                len_v = row.x; st_v = row.y;
                // int(L / sps) + (fraction > 0.5), as k_batch_bits takes it
                const uint32_t q = (uint32_t)(len_v < 0 ? -(int64_t)len_v : (int64_t)len_v), qq = q / c_sps, rr = q - qq * c_sps;
                nsym_v = len_v < 0 ? -(int)qq : (int)(qq + ((2 * (uint64_t)rr > (uint64_t)c_sps) ? 1u : 0u));
            }
            const int cnt_rows = (int)((nr - rb < 64) ? (nr - rb) : 64);
            for (int j = 0; j < cnt_rows; ++j) {
                const int64_t len = batch_lane(len_v, j), nsym = batch_lane(nsym_v, j);
                const int s = batch_lane(st_v, j);
                if (rb + j == 0 && s == -1) { ts += len; continue; }           // "starts with pause": only seeds total_samples
                if (s == -1 && !(nsym <= pt || pt == 0)) {                     // a long pause
                    if (there_was_data) {
                        REC_CLOSE(true, ts);
                        REC_LOAD_MSG();
                        there_was_data = false;
                    }
                    nb = 0; have_t = false;                                    // (without data: drops what was gathered)
                    ts += len;
                    continue;
                }
                const int64_t k_bits = nsym * c_bps;
                if (k_bits > 0) {
                    if (nb == 0) first = ts;
                    if (!have_t && t >= nb && t < nb + k_bits) { pos_t = ts + (t - nb) * spb; have_t = true; }
                    nb += k_bits;
                }
                if (s != -1 && !there_was_data && nsym > 0) there_was_data = true;
                ts += len;
            }
        }
        if (there_was_data) REC_CLOSE(false, ts);
#undef REC_CLOSE
#undef REC_LOAD_MSG
        if (m > n_msg) m = n_msg;
    }
    // what the sweep did not reach (all of a truncated or refused capture's): flag 0
    for (int64_t i = m + lane; i < n_msg; i += 64) rec_store(a, base + i, 0, 0, 0, 0, cap.src);
}

// EACH: the window is as long as the samples per symbol of the capture the message lies in (its record of a.b.each; no map: the capture itself)
template <int DT, bool EACH = false>
__global__ __launch_bounds__(kRecThreads) void k_batch_msg_records(const BatchRecArgs a) {
    __shared__ RecShared sh;
    const int tid = threadIdx.x;
    int64_t n_rec = a.rec_dir[a.b.k];
    if (n_rec > a.cap_rec) n_rec = a.cap_rec;
    for (int64_t i = blockIdx.x; i < n_rec; i += gridDim.x) {
        // ---- the record's window: Python's slice of the capture the message lies in (every thread alike) ----
        const int64_t mid = a.rec[i].mid_pos;
        const bool ok = a.rec[i].flag == 1;
        int64_t s0 = 0, n_c = 0, lo = 0, w = 0;
        const bool there = ok && rec_samples(a, a.rec_capture[i], &s0, &n_c);
        if constexpr (EACH) {                                                 // (rec_samples: the index lies inside [0, k))
            if (there) py_slice(mid, mid + (int64_t)a.b.each[a.rec_capture[i]].samples_per_symbol, n_c, &lo, &w);
        } else if (there) py_slice(mid, mid + (int64_t)a.b.sps, n_c, &lo, &w);       // lo + w <= n_c: no load leaves [start[c], start[c + 1])
        // ---- np.mean of the window's terms ----
        const double total = rec_window_sum<DT>(sh, a.b.iq, s0 + lo, w, a.norm);
        if (tid == 0) {
            const bool good = there && !sh.bad;
            a.rec[i].rssi = (good && w > 0) ? total / (double)w : __builtin_nan("");
            a.rec[i].flag = good ? 1 : (there ? -1 : 0);
        }
        __syncthreads();                                               // (the next message's round starts from a clean state)
    }
}


// ---- host side, defined in batch_records.hip ----
// k_batch_rec_dir: one launch
void launch_batch_rec_dir(const BatchRecArgs &a, hipStream_t s);

}  // namespace urh
