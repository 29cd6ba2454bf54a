// pass.hpp -- private to the units behind the C ABI (ctx / pass / stream_pass / shard / capi_* / probes .hip): how a capture is cut into
// chunks, the hot launch with its bookkeeping, and the single-GPU pass the other kinds of pass are built from.  Definitions: pass.hip.
#pragma once
#include <math.h>

#include <atomic>
#include <algorithm>
#include <new>
#include <vector>

#include "common.hpp"
#include "compact.hpp"
#include "launchers.hpp"

namespace urh {

struct Plan { int64_t n_chunks, chunk_len, slab_stride; };   // how a capture of n samples is cut into chunks
constexpr int kMaxWorld = 1024;   // ranks of a sharded capture (table entries reserved for their summaries)

extern bool g_tile_tail;              // test hooks, probes.hip
extern int g_force_tiles_per_chunk;

int check_params(const urhgpu_params *p, bool need_sps);
Plan make_plan(const urhgpu_ctx *ctx, int64_t n, int tol);
size_t digitize_scratch_bytes(const Plan &pl, int64_t cap_rows, bool ask, bool bits);
inline int value_bytes(int dtype) {                       // of one component of a sample; 0: no such dtype
    switch (dtype) {
        case URHGPU_DT_I8: case URHGPU_DT_U8: return 1;
        case URHGPU_DT_I16: case URHGPU_DT_U16: return 2;
        case URHGPU_DT_F32: return 4;
        default: return 0;
    }
}
inline int dtype_bytes(int dtype) { return 2 * value_bytes(dtype); }     // of one IQ sample
void hot_cu_mask(int removed, uint32_t mask[8]);          // ctx.hip
void free_shard_session(urhgpu_ctx *ctx);                // shard.hip
// the hot launch: one path for every kind of pass
int hot_run_args(const urhgpu_ctx *ctx, const urhgpu_params *p, const Plan &pl, int64_t n, int64_t pos_base, bool from_iq, RunArgs *a);
int hot_stream_begin(urhgpu_ctx *ctx, hipStream_t *out);
int hot_launch(urhgpu_ctx *ctx, const RunArgs &a, const urhgpu_params *p, bool from_iq, hipStream_t s, bool offer, hipEvent_t fallback,
               hipStream_t s_tail, hipEvent_t *hot_done);
void table_args(urhgpu_ctx *ctx, const urhgpu_params *p, const Plan &pl, int64_t n, ChunkInfo *chunks, uint64_t *slab, void *rs_mem, int64_t *rows,
                int64_t cap_rows, int64_t *d_n_acc, int64_t *d_n_rows, int64_t *d_n_rows_needed, bool ask, ResolveArgs *r, EmitArgs *e);
int tile_tail_mem(urhgpu_ctx *ctx, int64_t n_entries, bool expands_bits, TileTailMem *tm);
int scan_state(urhgpu_ctx *ctx, int64_t cap_rows, ScanState *out);
int reserve_rdesc(urhgpu_ctx *ctx, int64_t n_entries);
int reserve_auto_center_pass(urhgpu_ctx *ctx, int64_t n_max, int tolerance, int64_t cap_rows);
int reserve_pass_descriptors(urhgpu_ctx *ctx, int64_t n_max, int tolerance, int64_t cap_rows);
BitsParams bits_params(const urhgpu_params *p);
int begin_pipelined_pass(urhgpu_ctx *ctx);
int end_pipelined_pass(urhgpu_ctx *ctx);
int digitize(urhgpu_ctx *ctx, bool from_iq, const void *d_in, int64_t n, const urhgpu_params *p, float *d_qad, int64_t *d_rows, int64_t cap_rows,
             int64_t *d_n_rows, int64_t *d_n_rows_needed, int64_t *d_n_acc, const Plan &pl, int seg_mode = 0, hipStream_t s_tail = nullptr,
             const BitsParams *tile_bp = nullptr, TileTailMem *tile_out = nullptr, const float *d_thr = nullptr, const float *d_noise = nullptr);

// msg_estimators.hip: the center chain (detect_center of one range, queued, never waited for) behind the automatic center of a pass
struct CenterChain { void *d_st; unsigned int *d_hist; float *d_thr; };
size_t center_chain_bytes(int64_t n, int64_t max_bins);
int reserve_center_chain(urhgpu_ctx *ctx, int64_t n_max);
int center_chain_async(urhgpu_ctx *ctx, const float *d_x, int64_t n, int64_t max_size, hipStream_t s, CenterChain *out);
int center_publish(const CenterChain &c, const urhgpu_params *p, void *d_result, void *h_result, int64_t hist_cap, hipStream_t s);

}  // namespace urh
