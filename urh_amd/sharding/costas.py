"""PSK across the shards: the Costas loop carries its state {freq, phase} across the whole capture.  A PSK pass (orders 2 and 4) first runs
the loop across the shards, then the phases of the fused pass from the shard's demodulated signal:

    0. (no exchange) every rank > 0 is handed the `costas_halo_samples` raw samples before its shard (`left_raw`)
    1. speculate   candidate trajectories per 4096-sample chunk of the shard (the single-GPU kernels; chunk 0 warms
                   up in the halo), reduced to a 160-byte summary: chunk 0's candidate start states, the composition of
                   the shard's chunk maps, the last chunk's end states, "no un-gated sample"
    2. compose     all-gather the summaries; `costas_compose` (a pure function of the gathered bytes: every rank takes
                   the same branch) carries the state from {0, 1.5} across the shards by bitwise lookups.  Where it cannot,
                   the rank at the break resolves and hands its true end state over in one more all-gather of 8 bytes per
                   rank (`costas_exchange`: rounds <= world; one in the common case)
    3. resolve     every rank stitches from its true start state and writes its shard's qad
    4. halo        one all-gather of 4 bytes: every shard's last demodulated value (the seam of the pulse table), then
                   summary / rows / flags as in the fused pass (pipeline.py)."""
import numpy as np

from .comm import carry_across_ranks

COSTAS_SUMMARY_BYTES = 160                  # URHGPU_COSTAS_SUMMARY_BYTES
COSTAS_START = (0x00000000, 0x3FC00000)     # the loop's initial state {freq 0.0f, phase 1.5f} as float32 bits (signal_functions.pyx:261)
_COSTAS_WARM_BACK = 16                      # kWarmBackFactor (costas.hip): a candidate looks back at most 16 x its warm-up


def costas_halo_samples(bandwidth, pos_base=None):
    """urhgpu_costas_halo_samples: raw samples before its shard that a PSK rank > 0 is handed (`left_raw`) -- every sample the
    warm-up of its first chunk may read: 8 192 at bandwidth 0.1, up to 131 072 at the smallest bandwidths.  pos_base given: no more
    than the capture holds before the shard from sample 1 on (sample 0 is not part of the loop)."""
    want = 40.0 / max(1e-3, min(1.0, abs(float(np.float32(bandwidth)))))      # costas_warm (costas.hip), in double
    w = 256
    while w < want and w < 8192:
        w *= 2
    h = _COSTAS_WARM_BACK * w
    return h if pos_base is None else min(h, max(int(pos_base) - 1, 0))


def pack_costas_summary(starts, ends, cmap, reps, identity=False, n_chunks=1, ungated=None):
    """One Costas shard summary in the layout k_costas_shard_summary (costas.hip) writes: uint8 (COSTAS_SUMMARY_BYTES,).
    starts / ends: K states (freq bits, phase bits) of the first chunk's candidates / the last chunk's (None: not a representative);
    cmap: the composed chunk map (nibble k: last-chunk candidate of first-chunk candidate k, 0xF broken); reps: K flags."""
    w = np.zeros(COSTAS_SUMMARY_BYTES // 4, np.uint32)
    for k, s in enumerate(starts):
        w[2 * k], w[2 * k + 1] = s
    for k, e in enumerate(ends):
        if e is not None:
            w[16 + 2 * k], w[17 + 2 * k] = e
    w[32] = cmap
    w[33] = sum(1 << k for k, r in enumerate(reps) if r)
    w[34] = 1 if identity else 0
    w[35] = len(starts)
    w[36:38] = np.array([n_chunks], np.int64).view(np.uint32)
    w[38:40] = np.array([(0 if identity else 1) if ungated is None else ungated], np.int64).view(np.uint32)
    return w.view(np.uint8)


def costas_compose(summaries, handoff=None):
    """Carry the Costas loop state across the shards: a pure function of the gathered summaries ((world, COSTAS_SUMMARY_BYTES)
    bytes, rank order) and of the end states handed over so far (handoff: {rank: (freq bits, phase bits)}), so every rank that
    evaluates it takes the same branch.  Rank 0 starts in COSTAS_START; a shard without an un-gated sample passes the state on;
    otherwise the state is looked up BITWISE among the representatives of its first chunk's candidates and the composed map names
    the last-chunk candidate whose end state comes out.  Returns (starts, pending): starts[r] = the true state at the start of shard
    r as (freq bits, phase bits), None where not known yet; pending = the first rank whose end state the summaries cannot give (its
    start state is known: it resolves and hands its end state over), None when every start state is known."""
    raw = np.ascontiguousarray(np.asarray(summaries, dtype=np.uint8)).reshape(-1, COSTAS_SUMMARY_BYTES)
    w = raw.view("<u4")
    handoff = handoff or {}
    starts = [None] * len(w)
    state = COSTAS_START
    for r, row in enumerate(w):
        starts[r] = state
        if r in handoff:
            state = (int(handoff[r][0]), int(handoff[r][1]))
            continue
        if row[34]:
            continue                                  # gated samples freeze the loop: end state = start state
        K, reps, cmap = int(row[35]), int(row[33]), int(row[32])
        q = 0xF
        for k in range(min(K, 8)):
            if (reps >> k) & 1 and (int(row[2 * k]), int(row[2 * k + 1])) == state:
                q = (cmap >> (4 * k)) & 0xF
                break
        if q >= min(K, 8):                            # no candidate starts in the state, or the map is broken
            return starts, r
        state = (int(row[16 + 2 * q]), int(row[17 + 2 * q]))
    return starts, None


def costas_exchange(comm, summary, resolve, end_state):
    """Steps 2-3 of a PSK pass (module docstring): all-gather the summaries, compose, and let this rank resolve as soon as its start
    state is known; while the chain breaks at some rank, that rank's end state comes in one more all-gather (carry_across_ranks).
    summary: this rank's summary (uint8 tensor); resolve((freq bits, phase bits)) stitches this rank from its true start state;
    end_state(): 2 x int32 tensor, the rank's true end state once it has resolved.  Returns the number of rounds."""
    summaries = comm.all_gather(summary).cpu().numpy()
    resolved = []

    def on_starts(starts):
        if not resolved and starts[comm.rank] is not None:
            resolve(starts[comm.rank])
            resolved.append(True)
    return 1 + carry_across_ranks(comm, summaries, costas_compose, on_starts, lambda starts, pending: end_state())[1]
