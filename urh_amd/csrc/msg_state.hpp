// msg_state.hpp -- the per-range state of the estimator chains (msg_estimators.hip), shared with the translation units that read a chain's
// result on the device (batch_center.hip: k_batch_center_publish).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace urh {

constexpr int kMeTile = 4096;                 // samples per tile: 256 threads x 16 consecutive samples

struct MsgState {            // one per message, device resident between the stages (host mirror: same layout)
    int64_t start, end;      // sample range in the demodulated signal
    int64_t first_tile;      // index of its first tile in the tile table
    int64_t kept;            // samples > -4 (AutoInterpretation.py:227)
    int64_t a, L;            // trimmed range [a, a + L) of the kept samples (:231)
    float mn, mx;            // util.minmax of the trimmed samples (:236)
    float mean, var;         // float32 np.mean / np.var (:240)
    double e0, delta;        // bin edges e0 + i * delta (np.arange(min, max + step, step), :243)
    int64_t n_edges;         // 0: no histogram (empty, zero / NaN variance, fewer than 2 edges); > max_bins + 1: too many for the pool
    int64_t n_plateaus;      // urhgpu_msg_plateaus: plateaus found, -1: the window did not reach the 25 % mark
    int64_t edge_cnt;        // boundaries found in the window
    int64_t window;          // samples of the message searched for boundaries
    double center;           // center handed to urhgpu_msg_plateaus (NaN: none)
    double peak_center;      // urhgpu_msg_center_stats: center picked from the histogram (k_me_peaks)
    int64_t peak_flag;       // 0 none, 1 peak_center valid, 2 more bins than the pool holds, 3 equally populated peaks compete for a slot
    int64_t skip;            // 1: the message's first sample is filtered (x <= -4: afp_demod's result[0] = NOISE of FSK / PSK) -- k_me_first
    int64_t pairs_base;      // urhgpu_msg_plateau_decisions: first (value, count) pair of the message's plateau lengths in the pool ...
    int64_t pairs_n;         // ... and how many; -1: more distinct lengths than the table holds / the pool is full (the sequence decides)
    int64_t cut;             // detect_center's max_size (AutoInterpretation.py:233-234): 0 none, else max_size + 1 -- the trimmed range keeps its first max_size samples
};

// The center chain over the K captures of a batch (msg_estimators.hip "the center chain over the captures of a batch"): where a group's
// scratch lies in the caller's buffer -- host arithmetic shared by the size call and the launches (batch_center.hip)
struct BatchCenterScratch {
    int64_t group;           // captures per group: the group's histogram pool stays within kCenterBatchBytes
    int64_t n_groups;        // ceil(k / group)
    int64_t n_tiles;         // tile table entries of a group: total / kMeTile + min(k, group) + 1 -- an upper bound, the last one the spare range's
    size_t off_st, off_tiles, off_pre, off_mm, off_half, off_leaf, off_kept, off_wide, off_hist;
    size_t pool_bytes;       // the pool, any_wide and any_dirty: cleared with the per-tile counts behind it by ONE fill per group
    size_t bytes;
};
BatchCenterScratch batch_center_scratch(int64_t k, int64_t total, int64_t max_bins);
// the chain for the captures [c0, c0 + kg) of a batch, queued on s and never waited for: the states are built on the device from d_start (and the
// captures' noise flags, d_noise or nullptr), the existing chain kernels run on them, and the states and the folded histograms (row c - c0 of
// max_bins counters at *d_hist) stay in the scratch for k_batch_center_publish.  kBatchCenterChainLaunches launches and one fill, whatever kg is.
int center_stats_batch_async(const float *d_x, int64_t total, const int64_t *d_start, int64_t k, const void *d_noise, int64_t c0, int64_t kg,
                             int64_t max_size, int64_t max_bins, const BatchCenterScratch &L, char *scratch, hipStream_t s, MsgState **d_st,
                             unsigned int **d_hist);
constexpr int kBatchCenterChainLaunches = 13;

}  // namespace urh
