#!/usr/bin/env python3
"""One rank of a REAL multi-process PSK pass (launched by tests/test_psk_real_ranks.py through torch.distributed.run): every rank on
device 0, the process group over gloo (RCCL refuses two ranks on one device), the exchanges through TorchDistComm's host path.  Each
rank builds the same seeded capture, keeps its shard plus the raw halo before it, runs ShardedPipeline.iq_to_bits; rank 0 gathers the
pieces, compares the stitched result and the concatenated qad with the oracle over the whole capture -- bit-exact -- and prints
"PSK_SHARD_OK <world> rounds=<r>"."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import torch
    import torch.distributed as dist
    from test_costas_shard import params, psk_capture
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, TorchDistComm, costas_halo_samples, shard_bounds, stitch
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    n = 250_000
    iq, noise = psk_capture(n, 4, seed=404, gaps=((120_000, 133_000),))
    p = params(4, noise)
    a, b = shard_bounds(n, world)[rank]
    shard = torch.from_numpy(iq[a:b]).cuda()
    left = torch.from_numpy(iq[a - costas_halo_samples(p.costas_loop_bandwidth, a):a]).cuda() if rank else None
    pipe = ShardedPipeline(GpuShardEngine(0), TorchDistComm())
    res = pipe.iq_to_bits(shard, p, want_qad=True, pos_base=a, n_total=n, left_raw=left)
    torch.cuda.synchronize()
    piece = res.piece()
    piece["qad"] = res.qad.cpu().numpy()
    piece["rounds"] = pipe.last_costas["rounds"]
    pieces = [None] * world
    dist.all_gather_object(pieces, piece)
    if rank == 0:
        import urh_oracle as oracle
        qad = oracle.afp_demod(iq, noise, "PSK", 4, 0.1)
        qad[0] = -4.0
        pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, "PSK", 100, 2, p.center_spacing)
        flat = oracle.ppseq_to_bits_flat(pp, 100, 2, True, 8)
        got = stitch(pieces)
        assert np.array_equal(np.concatenate([pc["qad"] for pc in pieces]).view(np.uint32), qad.view(np.uint32)), "qad differs"
        assert np.array_equal(got[0], pp), "pulse table differs"
        for k in range(5):
            assert np.array_equal(got[1 + k], flat[k]), k
        assert len({pc["rounds"] for pc in pieces}) == 1, [pc["rounds"] for pc in pieces]
        print(f"PSK_SHARD_OK {world} rounds={pieces[0]['rounds']}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
