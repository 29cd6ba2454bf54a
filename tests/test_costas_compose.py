"""The composition step of a sharded PSK pass (urh_amd.sharding.costas_compose / costas_exchange) on hand-built Costas shard summaries:
no GPU.  The composition is a pure function of the gathered bytes: states are compared on their bits (last bits, signed zeros and NaN
payloads included), every rank gets the same answer, and a break at some rank costs one more round per break."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from urh_amd.sharding import (COSTAS_START, COSTAS_SUMMARY_BYTES, ThreadComm, costas_compose, costas_exchange, costas_halo_samples,
                              pack_costas_summary)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def st(freq, phase):
    return (bits(freq), bits(phase))



def chain(world, K=8, seed=0):
    """world shards where the state entering shard r is candidate k_r of its first chunk and leaves as candidate q_r's end state"""
    rng = np.random.default_rng(seed)
    states = [COSTAS_START] + [st(rng.uniform(-0.01, 0.01), rng.uniform(-6, 6)) for _ in range(world)]
    summ = []
    for r in range(world):
        k, q = int(rng.integers(0, K)), int(rng.integers(0, K))
        starts = [st(0.0, 1.5 + 1.5707964 * (j - K // 2) + 0.001 * r) for j in range(K)]
        starts[k] = states[r]
        ends = [None] * K
        ends[q] = states[r + 1]
        cmap = 0xFFFFFFFF & ~(0xF << (4 * k)) | (q << (4 * k))
        summ.append(pack_costas_summary(starts, ends, cmap, [True] * K, n_chunks=3))
    return np.stack(summ), states


def test_summary_layout():
    s = pack_costas_summary([COSTAS_START] * 4, [None, st(0.0, 1.0), None, None], 0x76543210, [1, 0, 0, 0], n_chunks=7, ungated=99)
    assert s.dtype == np.uint8 and s.shape == (COSTAS_SUMMARY_BYTES,)
    w = s.view(np.uint32)
    assert (w[0], w[1]) == COSTAS_START and w[33] == 1 and w[35] == 4 and w[34] == 0
    assert w[36:38].view(np.int64)[0] == 7 and w[38:40].view(np.int64)[0] == 99


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_chain_through_every_rank(world):
    summ, states = chain(world, seed=world)
    starts, pending = costas_compose(summ)
    assert pending is None
    assert starts == states[:world]


def test_identity_shard_passes_the_state_on():
    summ, states = chain(4, seed=5)
    # shard 2 has no un-gated sample: its candidates are unrelated, the state passes through unchanged
    summ[2] = pack_costas_summary([st(0.0, 9.0)] * 8, [None] * 8, 0xFFFFFFFF, [True] + [False] * 7, identity=True)
    # ... and shard 3 now has to start where shard 2 started
    s3 = summ[3].view(np.uint32).copy()
    k3 = next(k for k in range(8) if (int(s3[2 * k]), int(s3[2 * k + 1])) == states[3])
    s3[2 * k3], s3[2 * k3 + 1] = states[2]
    summ[3] = s3.view(np.uint8)
    starts, pending = costas_compose(summ)
    assert pending is None and starts == [states[0], states[1], states[2], states[2]]


def test_break_and_the_rounds_that_follow():
    summ, states = chain(6, seed=11)
    # shard 2: the incoming state is no candidate's (one ulp off); shard 4: the map is broken
    s2 = summ[2].view(np.uint32).copy()
    k2 = next(k for k in range(8) if (int(s2[2 * k]), int(s2[2 * k + 1])) == states[2])
    s2[2 * k2 + 1] += 1
    summ[2] = s2.view(np.uint8)
    s4 = summ[4].view(np.uint32).copy()
    s4[32] = 0xFFFFFFFF
    summ[4] = s4.view(np.uint8)
    starts, pending = costas_compose(summ)
    assert pending == 2 and starts[:3] == states[:3] and starts[3:] == [None] * 3
    starts, pending = costas_compose(summ, {2: states[3]})           # rank 2 resolved and handed its true end state over
    assert pending == 4 and starts[:5] == states[:5] and starts[5] is None
    starts, pending = costas_compose(summ, {2: states[3], 4: states[5]})
    assert pending is None and starts == states[:6]


def test_duplicate_candidates_take_the_representative():
    K = 8
    s = st(0.002, -2.5)
    starts = [st(0.0, 1.0 + j) for j in range(K)]
    starts[1] = starts[5] = s                                         # candidate 5 met candidate 1 during the warm-up
    reps = [True] * K
    reps[5] = False
    ends = [None] * K
    ends[6] = st(0.001, 0.25)
    cmap = 0xFFFFFFFF & ~(0xF << 4) | (6 << 4)                       # only the representative (1) carries a map entry
    summ = np.stack([pack_costas_summary([COSTAS_START] + [st(0.0, 3.0)] * 7, [None, s] + [None] * 6, 0xFFFFFFF1, [True] * 8),
                     pack_costas_summary(starts, ends, cmap, reps)])
    starts_out, pending = costas_compose(summ)
    assert pending is None and starts_out == [COSTAS_START, s]


@pytest.mark.parametrize("incoming, candidate, match", [
    ((bits(0.0), bits(1.5)), (bits(-0.0), bits(1.5)), False),          # signed zero: equal as floats, different bits
    ((bits(0.0), 0x7FC00001), (bits(0.0), 0x7FC00001), True),         # the same NaN payload: a match (NaN != NaN as floats)
    ((bits(0.0), 0x7FC00001), (bits(0.0), 0x7FC00002), False),        # another payload: none
    ((bits(0.001), bits(2.0)), (bits(0.001), bits(2.0) + 1), False),   # the last bit
    ((bits(0.001), bits(2.0)), (bits(0.001), bits(2.0)), True),
])
def test_states_compare_on_bits(incoming, candidate, match):
    end = st(0.0, 0.5)
    r0 = pack_costas_summary([COSTAS_START] * 8, [incoming] + [None] * 7, 0xFFFFFFF0, [True] + [False] * 7)
    r1 = pack_costas_summary([candidate] + [st(0.0, 4.0)] * 7, [end] + [None] * 7, 0xFFFFFFF0, [True] * 8)
    starts, pending = costas_compose(np.stack([r0, r1]))
    assert starts[1] == incoming
    assert (pending is None) == match


def test_order_two_summaries():
    K = 4
    starts = [COSTAS_START] * K
    summ = pack_costas_summary(starts, [st(0.0, 0.75)] + [None] * 3, 0xFFFFFFF0, [True, False, False, False])
    r1 = pack_costas_summary([st(0.0, 0.75)] + [st(0.0, 5.0)] * 3, [None, None, st(0.0, 0.1), None], 0xFFFFFFF2, [True] * K)
    starts_out, pending = costas_compose(np.stack([summ, r1]))
    assert pending is None and starts_out == [COSTAS_START, st(0.0, 0.75)]


def test_every_rank_gets_the_same_answer_and_rounds():
    """costas_exchange over ThreadComm (CPU tensors): every rank ends with the same number of all-gathers, the ranks at a break
    resolve first, and each rank resolves exactly once from its true start state"""
    world = 5
    summ, states = chain(world, seed=3)
    for broken in ([], [1], [1, 3], [0, 2, 4]):
        sm = summ.copy()
        for r in broken:
            w = sm[r].view(np.uint32).copy()
            w[32] = 0xFFFFFFFF
            sm[r] = w.view(np.uint8)
        shared = ThreadComm.Shared(world)
        rounds, got, err = [None] * world, [None] * world, []

        def work(r):
            try:
                end = torch.zeros(2, dtype=torch.int32)
                calls = []

                def resolve(start):
                    calls.append(start)
                    end.copy_(torch.from_numpy(np.array(states[r + 1], np.uint32).view(np.int32)))
                rounds[r] = costas_exchange(ThreadComm(shared, r), torch.from_numpy(sm[r].copy()), resolve, lambda: end)
                got[r] = calls
            except BaseException as e:                  # noqa: BLE001
                err.append(e)
                shared.barrier.abort()
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(60)
        assert not err and not any(t.is_alive() for t in ts), err
        assert rounds == [1 + len(broken)] * world, (broken, rounds)
        assert got == [[states[r]] for r in range(world)], broken


def test_halo_samples_match_the_library():
    from urh_amd import _lib
    from urh_amd.pipeline import DemodParams
    lib = _lib.load()
    for bw in (0.0, 1e-4, 0.001, 0.005, 0.01, 0.0123, 0.05, 0.1, 0.2, 0.5, 1.0, 3.0, -0.1, float("nan")):
        p = DemodParams("PSK", 2, 0.1, 0.0, 1.5, 5, 100, bw, 8, True).to_c(np.float32)
        assert lib.urhgpu_costas_halo_samples(C.byref(p)) == costas_halo_samples(bw), bw
    assert costas_halo_samples(0.1) == 8192 and costas_halo_samples(0.001) == 131072
    assert costas_halo_samples(0.1, pos_base=5000) == 4999 and costas_halo_samples(0.1, pos_base=10**6) == 8192


def test_psk_without_left_raw_raises_before_any_collective():
    """a rank > 0 without (or with too short) a halo raises ValueError naming the count, before its first collective"""
    from urh_amd.pipeline import DemodParams
    from urh_amd.sharding import ShardedPipeline

    class NoComm:
        rank, world = 1, 2

        def all_gather(self, t):
            raise AssertionError("a collective was entered")
        all_gather_start = all_gather

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was used: {name}")
    p = DemodParams("PSK", 2, 0.1, 0.0, 1.5, 5, 100, 0.1, 8, True)
    sp = ShardedPipeline(NoEngine(), NoComm())
    x = torch.zeros((50_000, 2), dtype=torch.float32)
    with pytest.raises(ValueError, match="8192"):
        sp.iq_to_bits(x, p, pos_base=50_000, n_total=100_000)
    with pytest.raises(ValueError, match="8192"):
        sp.iq_to_bits(x, p, pos_base=50_000, n_total=100_000, left_raw=torch.zeros((8191, 2)))
    with pytest.raises(ValueError, match="2999"):
        sp.iq_to_bits(x, p, pos_base=3000, n_total=100_000, left_raw=torch.zeros((100, 2)))
