"""Sample-contiguous sharding of one long capture over the GPUs of a node.

Rank r holds samples [r*n_local, (r+1)*n_local) of the capture (the last rank may hold more or
fewer).  The hot kernel runs on every shard independently; what crosses a shard boundary is tiny and
is exchanged with three (ASK: four) small all-gathers -- no data-path collective ever moves samples:

    1. halo        the last two IQ samples of every shard (16 B)      -> seam of the FSK conj-product and
                                                                        the state of the sample before the shard
    2. summary     one ChunkInfo (72 B) per shard: the shard's run structure reduced to what its
                   neighbours need (leading run length, first / last stable run, still-short trailing run,
                   number of accepted runs)                           -> pulse-table rows with global lengths
    3. (ASK only)  first / last row of every shard's merged table     -> equal-state rows merged across shards
    4. bits        three flags per shard (long pause present, data before the first / after the last one)
                                                                      -> which boundary-spanning groups are messages

The result stays sharded: rank r owns the pulse-table rows that END in its shard and the bits /
bit_sample_pos those rows expand to; concatenating the ranks' pieces in rank order gives exactly the
single-GPU (and reference) result (`stitch`).

Which module says how:
    pipeline.py   ShardedPipeline (one rank's orchestration of every pass), the estimators and the automatic passes, shard_bounds, stitch
    comm.py       the communicators (torch.distributed, RCCL direct, threads), counting all-gathers, carrying a state across the ranks
    costas.py     PSK: the Costas loop's state across the shards
    dc.py         DC correction: numpy's sequential float32 sum across the shards
    pairwise.py   the estimators: numpy's pairwise float32 sum, min / max and the trimmed sequence from the ranks' records
    records.py    message records: the first message of every rank, its positions and its window
"""
from .comm import RcclComm, ThreadComm, TorchDistComm, _CountingComm, carry_across_ranks
from .costas import _COSTAS_WARM_BACK, COSTAS_START, COSTAS_SUMMARY_BYTES, costas_compose, costas_exchange, costas_halo_samples, pack_costas_summary
from .dc import DC_IDENTITY, _dc_exit, dc_compose
from .pairwise import (HIST_GATHER_BINS, PW_LEAF, PW_PIECE, PW_REC_FIRST, PW_REC_HEAD, PW_REC_LAST, PW_REC_PIECES, PW_REC_TAIL, _record_headers, center_parts,
                       minmax_combine, pairwise_combine, pairwise_inside_pieces, pairwise_leaf_sum, pairwise_piece_leaves, pairwise_record_words,
                       pairwise_tree)
from .pipeline import ShardedPipeline, shard_bounds, stitch
from .records import (REC_FIRST_PAUSE, REC_FIRST_WORDS, REC_HEAD_BITS, REC_HEAD_POS, REC_HELD, REC_N_LOCAL, REC_N_MSG, REC_N_POS, REC_POS_BASE,
                      REC_SUMMARY_WORDS, REC_TAIL_BITS, REC_TAIL_POS, _py_slice, message_data, records_plan, records_requests, records_windows, stitch_records)
