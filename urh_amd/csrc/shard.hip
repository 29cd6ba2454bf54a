// shard.hip -- sharded captures (urhgpu_shard_*): one rank's phases; the all-gathers in between belong to the caller.
#include "pass.hpp"

using namespace urh;

namespace {

// State of one sharded pass (urhgpu_shard_*): lives in the context between the phases; every pointer is
// carved from ctx->arena, which is not reset until the next pass begins.
struct ShardSession {
    int phase = 0;                 // -1: hot launch without the first chunk, -2: whole hot launch; 1: runs done, 2: rows done, 3: bits prepared
    bool piped = false;            // pipelined mode: phases after the hot kernel run on ctx->tail_stream
    RunArgs run;                   // kernel arguments of the hot launch (kept for the deferred first chunk)
    int rank = 0, world = 1;
    int64_t n_local = 0, pos_base = 0, n_total = 0;
    urhgpu_params p;
    urhgpu_outputs out;
    Plan pl;
    ChunkInfo *table = nullptr;    // [world - 1 summaries interleaved | local chunks], see shard_rows
    uint64_t *slab = nullptr;
    ResolveAux *aux = nullptr;
    void *rs_mem = nullptr;
    int64_t *rows_stage = nullptr; void *merge_scratch = nullptr; int64_t *d_n_stage = nullptr;
    void *bits_scratch = nullptr;
    int64_t *d_small = nullptr;    // [0] ts_carry, [1] absorbed, [2] extra (2 x int32), [3] n_rows (final), [4] row_base (tile tail)
    const int64_t *d_row_base = nullptr;
    bool use_tile = false;         // everything but ASK: the tile tail over the table (pulse_table.hip), as on a single GPU
    TileTailMem tile;
    // PSK: the rank's Costas pass (urhgpu_shard_costas_*), whose output the runs phase reads instead of the IQ
    CostasShard costas;
    int costas_phase = 0;          // 1: speculated (summary out), 2: resolved (the shard's qad written), 0: none / taken by the runs phase
    // ASK / FSK: the demodulation phase (urhgpu_shard_demod_dev), after which the runs phase segments the shard's qad like a PSK pass
    bool demod_done = false;       // the shard's qad is written, for exactly the buffers and the gate below; taken by the runs phase
    const void *demod_iq = nullptr; float *demod_qad = nullptr; int64_t demod_n = 0;
    int demod_mod = 0, demod_dtype = 0; float demod_noise = 0.f;
    float *d_seam = nullptr;       // device float of the session: afp_demod's value of global sample pos_base - 1 (the left halo of the segmentation)
};

ShardSession *session(urhgpu_ctx *ctx) {
    if (!ctx->shard) ctx->shard = new (std::nothrow) ShardSession();
    return (ShardSession *)ctx->shard;
}

// the shard's place in the capture, as every entry point that opens a pass checks it: min_total is the shortest capture the route takes,
// min_base_later_ranks the samples a rank > 0 needs in front of its shard
int check_shard_geometry(int world, int rank, int64_t n_local, int64_t pos_base, int64_t n_total, int64_t min_total, int64_t min_base_later_ranks) {
    if (world < 1 || world > kMaxWorld || rank < 0 || rank >= world || n_local < 2 || pos_base < 0 || pos_base + n_local > n_total ||
        n_total < min_total)
        return URHGPU_ERR_ARG;
    return (rank == 0 ? pos_base != 0 : pos_base < min_base_later_ranks) ? URHGPU_ERR_ARG : URHGPU_OK;
}

// the stream of the phases behind the hot kernel
hipStream_t tail_stream_of(const urhgpu_ctx *ctx, const ShardSession *ss) { return ss->piped ? ctx->tail_stream : ctx->stream; }

// what bits_prepare and bits_finish tell the expansion kernels about this rank's place in the table
BitsParams shard_bits_params(const ShardSession *ss) {
    BitsParams bp = bits_params(&ss->p);
    bp.d_row_base = ss->d_row_base; bp.d_ts_carry = ss->use_tile ? nullptr : ss->d_small;
    bp.d_absorbed = (ss->p.mod == URHGPU_MOD_ASK) ? ss->d_small + 1 : nullptr;
    bp.d_extra = (const int32_t *)(ss->d_small + 2); bp.is_last_rank = (ss->rank == ss->world - 1) ? 1 : 0;
    return bp;
}

}  // namespace

void urh::free_shard_session(urhgpu_ctx *ctx) {
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (ss && ss->d_seam) (void)hipFree(ss->d_seam);
    delete ss;
    ctx->shard = nullptr;
}

extern "C" {

// ---- sharded captures (one rank's phases; the all-gathers in between belong to the caller) --------------
// validation + scratch + kernel arguments of a shard pass; launches the chunks selected by `part` on the hot stream
static int shard_launch(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, int rank, int world,
                        const void *d_left_halo, const urhgpu_params *p, const urhgpu_outputs *out, int part) {
    if (!ctx || !p || !out || !d_iq || !out->rows || !out->counts) return URHGPU_ERR_ARG;
    URH_TRY(check_shard_geometry(world, rank, n_local, pos_base, n_total, 0, 0));
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_TRY(check_params(p, true));
    if (((uintptr_t)d_iq & 15) || (out->qad && ((uintptr_t)out->qad & 7))) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    ShardSession *ss = session(ctx);
    if (!ss) return URHGPU_ERR_ARG;
    // PSK: the runs are segmented from the shard's Costas output (resolved by urhgpu_shard_costas_resolve_dev), the route of a
    // single-GPU PSK pass (digitize from qad); the halo is the previous shard's last demodulated value
    const bool psk = (p->mod == URHGPU_MOD_PSK);
    if (psk && (ctx->pipelined || part != 0)) return URHGPU_ERR_UNSUPPORTED;
    if (psk && (ss->costas_phase != 2 || out->qad != ss->costas.out || n_local != ss->costas.n || d_iq != ss->costas.iq)) return URHGPU_ERR_ARG;
    // ASK / FSK behind urhgpu_shard_demod_dev, for exactly the buffers and the gate it demodulated with: the same route, the halo being the
    // session's seam value.  Without that state: the fused hot kernel, as ever.
    const bool dem = !psk && part == 0 && !ctx->pipelined && ss->demod_done && out->qad && out->qad == ss->demod_qad && n_local == ss->demod_n &&
                     d_iq == ss->demod_iq && p->mod == ss->demod_mod && p->dtype == ss->demod_dtype && p->noise_threshold == ss->demod_noise;
    ss->demod_done = false;
    const bool from_qad = psk || dem;
    if (dem) d_left_halo = (rank > 0) ? (const void *)ss->d_seam : nullptr;
    ss->piped = ctx->pipelined;
    if (ss->piped) URH_TRY(begin_pipelined_pass(ctx)); else URH_TRY(join_tail(ctx));
    // ASK passes (generic tail: a dozen under-occupied launches and one more exchange) keep the caller's stream for the hot kernel and
    // 33 KiB of LDS padding per hot workgroup; everything else runs as on a single GPU: tile tail, CU-masked hot stream for float32
    // captures (measured on a 1-rank RCCL group, round 3: the generic tail ran 0.35-0.36 ms per pass with either, 0.40 with both)
    const bool ask = (p->mod == URHGPU_MOD_ASK);
    ss->use_tile = !ask && g_tile_tail;
    hipStream_t s = ctx->stream;
    if (ss->piped && ss->use_tile) URH_TRY(hot_stream_begin(ctx, &s));
    ss->phase = 0; ss->rank = rank; ss->world = world; ss->n_local = n_local; ss->pos_base = pos_base; ss->n_total = n_total;
    ss->p = *p; ss->out = *out;
    const Plan pl = make_plan(ctx, n_local, p->tolerance);
    ss->pl = pl;
    URH_TRY(ctx->arena.reserve(digitize_scratch_bytes(pl, out->cap_rows, ask, true)));
    ctx->arena.reset();
    const int64_t n_table = pl.n_chunks + world - 1;
    ss->table = (ChunkInfo *)ctx->arena.take((size_t)n_table * sizeof(ChunkInfo));
    ss->slab = (uint64_t *)ctx->arena.take((size_t)pl.n_chunks * pl.slab_stride * 8);
    ss->rs_mem = ctx->arena.take(resolve_scratch_bytes(n_table));
    ss->aux = (ResolveAux *)(ctx->d_tickets + 4);
    ss->d_small = (int64_t *)ctx->arena.take(8 * 8);
    ss->bits_scratch = ctx->arena.take(bits_scratch_bytes(std::max<int64_t>(out->cap_rows, 1)));
    ss->rows_stage = out->rows; ss->merge_scratch = nullptr; ss->d_n_stage = ss->d_small + 3;
    if (ask) {
        ss->rows_stage = (int64_t *)ctx->arena.take((size_t)out->cap_rows * 16);
        ss->merge_scratch = ctx->arena.take(merge_scratch_bytes(out->cap_rows));
        ss->d_n_stage = (int64_t *)ctx->arena.take(64);
    }
    if (!ss->table || !ss->slab || !ss->rs_mem || !ss->d_small || !ss->bits_scratch || !ss->rows_stage ||
        !ss->d_n_stage || (ask && !ss->merge_scratch))
        return URHGPU_ERR_ARG;
    if (ss->use_tile) {
        URH_TRY(tile_tail_mem(ctx, n_table, true, &ss->tile));
        if (world > 1) ss->tile.d_row_base = ss->d_small + 4;
    }
    RunArgs &a = ss->run;
    URH_TRY(hot_run_args(ctx, p, pl, n_local, pos_base, !from_qad, &a));       // (the qad-input routes read the shard's qad: no max_magnitude)
    a.in = from_qad ? (const void *)out->qad : d_iq; a.qad = from_qad ? nullptr : out->qad; a.left_halo = d_left_halo;
    a.lds_pad = !ctx->pipelined ? 0 : (ss->use_tile ? ctx->hot_lds_pad : ctx->hot_lds_pad_sharded);
    a.chunks = ss->table + rank;               // this rank's chunks sit at table[rank .. rank + n_chunks)
    a.slab = ss->slab;
    a.launch_part = part;
    if (part == 1 && rank > 0 && !a.left_halo) a.left_halo = d_iq;    // any non-null value: only chunk 0 reads the halo
    // Pipelined: what the tail stream waits for as in digitize.  Everything after this launch goes to the tail stream -- also the first
    // chunk of a prelaunched pass, which waits for the halo exchange: the caller's stream never waits for a collective (the exchanges
    // of one communicator run in issue order, so the halo of pass i + 1 queues behind the last exchange of pass i's tail).
    URH_TRY(hot_launch(ctx, a, p, !from_qad, s, ss->piped && n_local % kTile == 0, ss->piped ? ctx->ev_hot : nullptr,
                       ss->piped ? ctx->tail_stream : nullptr, nullptr));
    ss->costas_phase = 0;
    URH_HIP(hipGetLastError());
    return URHGPU_OK;
}

int urhgpu_shard_prelaunch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                               int rank, int world, const urhgpu_params *p, const urhgpu_outputs *out) {
    if (p && p->mod == URHGPU_MOD_PSK) return URHGPU_ERR_UNSUPPORTED;    // PSK: urhgpu_shard_costas_* first, then urhgpu_shard_runs_dev
    if (ctx && ctx->shard) ((ShardSession *)ctx->shard)->demod_done = false;     // the fused hot kernel was asked for
    URH_TRY(shard_launch(ctx, d_iq, n_local, pos_base, n_total, rank, world, nullptr, p, out, rank > 0 ? 1 : 0));
    ((ShardSession *)ctx->shard)->phase = -1;
    return URHGPU_OK;
}

int urhgpu_shard_launch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                            int rank, int world, const void *d_left_halo, const urhgpu_params *p, const urhgpu_outputs *out) {
    if ((rank == 0) != (d_left_halo == nullptr)) return URHGPU_ERR_ARG;
    if (p && p->mod == URHGPU_MOD_PSK) return URHGPU_ERR_UNSUPPORTED;    // PSK: urhgpu_shard_costas_* first, then urhgpu_shard_runs_dev
    if (ctx && ctx->shard) ((ShardSession *)ctx->shard)->demod_done = false;     // the fused hot kernel was asked for
    URH_TRY(shard_launch(ctx, d_iq, n_local, pos_base, n_total, rank, world, d_left_halo, p, out, 0));
    ((ShardSession *)ctx->shard)->phase = -2;
    return URHGPU_OK;
}

int urhgpu_shard_runs_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                          int rank, int world, const void *d_left_halo, const urhgpu_params *p,
                          const urhgpu_outputs *out, void *d_summary) {
    if (!ctx || !d_summary) return URHGPU_ERR_ARG;
    if ((rank == 0) != (d_left_halo == nullptr)) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    hipStream_t s;
    if (ss && (ss->phase == -1 || ss->phase == -2)) {
        // prelaunched: only the first chunk (it needs the halo) is still missing, or (-2) nothing
        if (ss->rank != rank || ss->world != world || ss->n_local != n_local || ss->run.in != d_iq) return URHGPU_ERR_ARG;
        URH_HIP(hipSetDevice(ctx->device));
        s = tail_stream_of(ctx, ss);
        if (rank > 0 && ss->phase == -1) {
            RunArgs a = ss->run;
            a.left_halo = d_left_halo; a.launch_part = 2;
            URH_TRY(launch_demod_runs_iq(a, p->dtype, p->mod, out->qad != nullptr, s));
        }
    } else {
        URH_TRY(shard_launch(ctx, d_iq, n_local, pos_base, n_total, rank, world, d_left_halo, p, out, 0));
        ss = (ShardSession *)ctx->shard;
        s = tail_stream_of(ctx, ss);      // pipelined: shard_launch made the tail stream wait for the hot kernel
    }
    // local resolve pass: the shard on its own -> its summary
    const Plan &pl = ss->pl;
    const int64_t n_table = pl.n_chunks + world - 1;
    ResolveArgs r;
    memset(&r, 0, sizeof(r));
    r.sc = resolve_scratch_carve(ss->rs_mem, n_table);
    r.chunks = ss->table + rank; r.n_chunks = pl.n_chunks; r.n_total = n_local; r.tol = ss->p.tolerance;
    r.rows = nullptr; r.cap_rows = 0; r.d_n_acc = ctx->d_counts + 9; r.d_n_rows = ctx->d_counts + 10;
    r.d_n_rows_needed = ctx->d_counts + 8; r.write_last_row = 0;
    r.local_pass = 1; r.aux = ss->aux; r.summary_out = (ChunkInfo *)d_summary; r.chunk_first = 0; r.n_local = pl.n_chunks;
    // one launch (k_shard_summary) since round 6; the three generic resolve launches stay as tuning key shard_summary_generic (tests compare the two)
    if (ctx->tune_shard_summary_generic) URH_TRY(launch_resolve(r, ctx->d_tickets, s));
    else URH_TRY(launch_shard_summary(r, ctx->d_tickets + 1, s));
    URH_HIP(hipGetLastError());
    ss->phase = 1;
    return URHGPU_OK;
}

// ---- ASK / FSK: the demodulation phase on its own (include/urhgpu.h) ----------------------------------------------------------------
int urhgpu_shard_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, int rank, int world,
                           const void *d_left_halo, const urhgpu_params *p, const urhgpu_outputs *out) {
    if (!ctx || !p || !out || !d_iq || !out->qad || !out->rows || !out->counts) return URHGPU_ERR_ARG;
    URH_TRY(check_shard_geometry(world, rank, n_local, pos_base, n_total, 3, 1));
    if ((rank == 0) != (d_left_halo == nullptr)) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    if (p->mod != URHGPU_MOD_ASK && p->mod != URHGPU_MOD_FSK) return URHGPU_ERR_UNSUPPORTED;      // (PSK has its Costas phases)
    URH_TRY(check_params(p, true));
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)out->qad & 7)) return URHGPU_ERR_ARG;
    if (ctx->pipelined) return URHGPU_ERR_UNSUPPORTED;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    ShardSession *ss = session(ctx);
    if (!ss) return URHGPU_ERR_ARG;
    ss->demod_done = false;
    ss->costas_phase = 0;
    ss->phase = 0;                                           // (a pass left behind its hot launch is over: the runs phase starts a new one)
    if (!ss->d_seam) URH_HIP(hipMalloc((void **)&ss->d_seam, 64));
    // rows [pos_base, pos_base + n_local) of afp_demod(whole capture): sample 0 of rank 0 is NOISE, a later rank's first FSK value comes from the
    // halo's last sample; whole chunks of 8192 through the streaming kernel, the remainder through k_afp_demod (launch_afp_demod)
    RunArgs a;
    URH_TRY(hot_run_args(ctx, p, make_plan(ctx, n_local, p->tolerance), n_local, pos_base, true, &a));
    a.in = d_iq; a.qad = out->qad; a.left_halo = d_left_halo;
    const int64_t rows = (n_local + 511) / 512;
    const int grid = (int)std::min<int64_t>(rows, (int64_t)ctx->prop.multiProcessorCount * 16);
    URH_TRY(launch_afp_demod(a, p->dtype, p->mod, grid, ctx->stream));
    if (rank > 0) URH_TRY(launch_afp_seam(a, p->dtype, p->mod, ss->d_seam, ctx->stream));
    URH_HIP(hipGetLastError());
    ss->demod_iq = d_iq; ss->demod_qad = out->qad; ss->demod_n = n_local;
    ss->demod_mod = p->mod; ss->demod_dtype = p->dtype; ss->demod_noise = p->noise_threshold;
    ss->demod_done = true;
    return URHGPU_OK;
}

int urhgpu_shard_seam_value(urhgpu_ctx *ctx, float *seam) {
    if (!ctx || !seam) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (!ss || !ss->d_seam) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_HIP(hipMemcpyAsync(seam, ss->d_seam, sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    URH_HIP(hipStreamSynchronize(ctx->stream));
    return URHGPU_OK;
}

int urhgpu_shard_rows_dev(urhgpu_ctx *ctx, const void *d_summaries, int64_t *d_merge) {
    if (!ctx || !d_summaries) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (!ss || ss->phase != 1) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = tail_stream_of(ctx, ss);
    const int rank = ss->rank, world = ss->world;
    const Plan &pl = ss->pl;
    const bool ask = (ss->p.mod == URHGPU_MOD_ASK);
    if (ask && !d_merge) return URHGPU_ERR_ARG;
    const int64_t n_table = pl.n_chunks + world - 1;
    const ChunkInfo *S = (const ChunkInfo *)d_summaries;
    // table = [S_0 .. S_{rank-1} | local chunks | S_{rank+1} .. S_{world-1}]
    if (rank > 0) URH_HIP(hipMemcpyAsync(ss->table, S, (size_t)rank * sizeof(ChunkInfo), hipMemcpyDeviceToDevice, s));
    if (rank + 1 < world)
        URH_HIP(hipMemcpyAsync(ss->table + rank + pl.n_chunks, S + rank + 1, (size_t)(world - 1 - rank) * sizeof(ChunkInfo),
                               hipMemcpyDeviceToDevice, s));
    ResolveArgs r;
    memset(&r, 0, sizeof(r));
    r.sc = resolve_scratch_carve(ss->rs_mem, n_table);
    r.chunks = ss->table; r.n_chunks = n_table; r.n_total = ss->n_total; r.tol = ss->p.tolerance;
    r.rows = ss->rows_stage; r.cap_rows = ss->out.cap_rows; r.d_n_acc = ctx->d_counts + 9; r.d_n_rows = ss->d_n_stage;
    r.d_n_rows_needed = ctx->d_counts + 8; r.write_last_row = (rank == world - 1) ? 1 : 0;
    r.local_pass = 0; r.aux = ss->aux; r.summary_out = nullptr; r.chunk_first = rank; r.n_local = pl.n_chunks;
    r.d_ts_carry = ss->d_small;
    URH_HIP(hipMemsetAsync(ss->d_small, 0, 8 * 8, s));
    EmitArgs e;
    e.sc = r.sc;
    e.chunks = ss->table; e.chunk_first = rank; e.slab = ss->slab; e.slab_stride = pl.slab_stride;
    e.rows = ss->rows_stage; e.cap_rows = ss->out.cap_rows; e.d_ts_carry = ss->d_small; e.is_ask = ask ? 1 : 0;
    e.sps = ss->p.samples_per_symbol;
    if (ss->use_tile) {
        // resolve + rows + per-tile bit aggregates over the table: two launches (total_samples before my first row comes out of the
        // tile scan, the summaries being tiles of their own: no ts_carry)
        BitsParams bp = bits_params(&ss->p);
        bp.d_row_base = ss->tile.d_row_base;
        URH_TRY(launch_tile_rows(r, e, ss->tile, &bp, s));
        ss->d_row_base = ss->tile.d_row_base;
    } else {
        URH_TRY(launch_resolve(r, ctx->d_tickets, s));
        URH_TRY(launch_emit_rows(e, pl.n_chunks, s));
        ss->d_row_base = r.sc.out_off + rank;
    }
    if (ask) {
        URH_TRY(launch_merge_rows_ask(ss->rows_stage, ss->d_n_stage, ss->out.cap_rows, ss->out.rows, ss->out.cap_rows,
                                      ss->d_small + 3, ss->merge_scratch, ctx->d_tickets, s));
        launch_merge_summary(ss->out.rows, ss->d_small + 3, d_merge, s);
    }
    URH_HIP(hipGetLastError());
    ss->phase = 2;
    return URHGPU_OK;
}

int urhgpu_shard_bits_prepare_dev(urhgpu_ctx *ctx, const int64_t *d_merge_all, int64_t *d_flags) {
    if (!ctx || !d_flags) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (!ss || ss->phase != 2) return URHGPU_ERR_ARG;
    const bool ask = (ss->p.mod == URHGPU_MOD_ASK);
    if (ask && !d_merge_all) return URHGPU_ERR_ARG;
    if (!ss->out.bits || !ss->out.msg_off || !ss->out.pauses || !ss->out.pos_off) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = tail_stream_of(ctx, ss);
    int64_t *d_n_rows = ss->d_small + 3;
    if (ask) launch_merge_fix(ss->out.rows, d_n_rows, d_merge_all, ss->rank, ss->world, ss->d_small + 1, s);
    const BitsParams bp = shard_bits_params(ss);
    ScanState sst;
    const int64_t cap = std::max<int64_t>(ss->out.cap_rows, 1);
    if (ss->use_tile) {
        URH_TRY(scan_state(ctx, tile_desc_cap(cap, ss->tile.n_chunks), &sst));
        URH_TRY(launch_tile_bits_prepare(ss->tile, ss->out.rows, d_n_rows, cap, bp, ss->bits_scratch, d_flags, sst, s));
    } else {
        URH_TRY(scan_state(ctx, cap, &sst));
        URH_TRY(launch_bits_prepare(ss->out.rows, d_n_rows, cap, bp, ss->bits_scratch, d_flags, sst, s));
    }
    URH_HIP(hipGetLastError());
    ss->phase = 3;
    return URHGPU_OK;
}

int urhgpu_shard_bits_finish_dev(urhgpu_ctx *ctx, const int64_t *d_flags_all) {
    if (!ctx || !d_flags_all) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (!ss || ss->phase != 3) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    hipStream_t s = tail_stream_of(ctx, ss);
    launch_bits_extra(d_flags_all, ss->rank, ss->world, (int32_t *)(ss->d_small + 2), s);
    BitsParams bp = shard_bits_params(ss);
    bp.d_rows_needed = ctx->d_counts + 8;
    const urhgpu_outputs &o = ss->out;
    BitsOut bo{o.bits, o.cap_bits, o.msg_off, o.pauses, o.cap_msg, o.pos, o.cap_pos, o.pos_off, o.counts};
    ScanState sst;
    const int64_t cap = std::max<int64_t>(o.cap_rows, 1);
    if (ss->use_tile) {
        URH_TRY(scan_state(ctx, tile_desc_cap(cap, ss->tile.n_chunks), &sst));
        URH_TRY(launch_tile_bits_finish(ss->tile, o.rows, ss->d_small + 3, cap, bp, bo, ss->bits_scratch, sst, s));
    } else {
        URH_TRY(scan_state(ctx, cap, &sst));
        URH_TRY(launch_bits_finish(o.rows, ss->d_small + 3, cap, bp, bo, ss->bits_scratch, sst, s));
    }
    if (o.blob) {
        // the compact mirror of this rank's piece (compact.hip); an absorbed first row (ASK) is shipped as state -128
        URH_TRY(launch_pack_blob(&o, ss->p.write_bit_sample_pos, s));
    }
    URH_HIP(hipGetLastError());
    ss->phase = 0;
    if (ss->piped) URH_TRY(end_pipelined_pass(ctx));
    return URHGPU_OK;
}

// ---- PSK across shards: the rank's Costas pass in two phases around the summary exchange (include/urhgpu.h) ----------------------
int64_t urhgpu_costas_halo_samples(const urhgpu_params *p) {
    if (!p) return 0;
    return costas_halo_samples(p);
}

int urhgpu_shard_costas_spec_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, int rank, int world,
                                 const void *d_halo, int64_t n_halo, const urhgpu_params *p, const urhgpu_outputs *out, void *d_summary) {
    if (!ctx || !p || !out || !d_iq || !out->qad || !d_summary) return URHGPU_ERR_ARG;
    URH_TRY(check_shard_geometry(world, rank, n_local, pos_base, n_total, 3, 2));
    if (p->mod != URHGPU_MOD_PSK) return URHGPU_ERR_ARG;
    if (dtype_bytes(p->dtype) == 0) return URHGPU_ERR_DTYPE;
    URH_TRY(check_params(p, true));
    if (((uintptr_t)d_iq & 15) || ((uintptr_t)out->qad & 7)) return URHGPU_ERR_ARG;
    if (ctx->pipelined) return URHGPU_ERR_UNSUPPORTED;
    // the halo: every sample a walk back of chunk 0 may read -- all of them down to global sample 1 where the capture starts closer
    const int64_t need = (rank == 0) ? 0 : std::min<int64_t>(costas_halo_samples(p), pos_base - 1);
    if (rank == 0 ? (d_halo != nullptr || n_halo != 0) : (d_halo == nullptr || n_halo < need || n_halo > pos_base)) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(join_tail(ctx));
    ShardSession *ss = session(ctx);
    if (!ss) return URHGPU_ERR_ARG;
    ss->costas_phase = 0;
    ss->demod_done = false;
    CostasShard &cs = ss->costas;
    cs.iq = d_iq; cs.n = n_local; cs.out = out->qad; cs.p = *p;
    cs.origin = (rank == 0) ? 1 : 0;
    cs.halo_end = (rank == 0) ? nullptr : (const char *)d_halo + (size_t)n_halo * dtype_bytes(p->dtype);
    cs.lo = (rank == 0) ? 1 : std::max<int64_t>(1 - pos_base, -n_halo);
    cs.start1 = 1 - pos_base;
    URH_TRY(ctx->aux.reserve(costas_scratch_bytes(n_local) + 1024));
    ctx->aux.reset();
    cs.scratch = ctx->aux.take(costas_scratch_bytes(n_local));
    if (!cs.scratch) return URHGPU_ERR_ARG;
    URH_TRY(launch_costas_shard_spec(ctx, cs, d_summary));
    ss->costas_phase = 1;
    return URHGPU_OK;
}

int urhgpu_shard_costas_resolve_dev(urhgpu_ctx *ctx, const uint32_t *start_state, uint32_t *d_end_state) {
    if (!ctx || !start_state) return URHGPU_ERR_ARG;
    ShardSession *ss = (ShardSession *)ctx->shard;
    if (!ss || ss->costas_phase != 1) return URHGPU_ERR_ARG;
    URH_HIP(hipSetDevice(ctx->device));
    URH_TRY(launch_costas_shard_resolve(ctx, ss->costas, start_state[0], start_state[1], d_end_state));
    ss->costas_phase = 2;
    return URHGPU_OK;
}

}  // extern "C"
