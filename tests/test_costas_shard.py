"""PSK captures sharded over W ranks -- threads on the one GPU, one GpuShardEngine each, ThreadComm (urh_amd/sharding.py, the PSK
pass): the Costas loop stitched across shard boundaries.  Every stitched result must equal the single-GPU DevicePipeline.iq_to_bits
result bit for bit -- qad (index 0 included: -4.0 on both), pulse table, bits, pauses, bit_sample_pos, offsets -- and the oracle
(afp_demod / grab_pulse_lens / ppseq_to_bits_flat) where the capture is small enough."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORACLE_MAX = 300_000


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def pipe():
    from urh_amd.pipeline import DevicePipeline
    return DevicePipeline()


@pytest.fixture(scope="module")
def engines():
    from urh_amd.shard_engine import GpuShardEngine
    return [GpuShardEngine(0) for _ in range(10)]


def psk_capture(n, order, seed, dtype=np.float32, gaps=(), offset=0.04):
    """seeded PSK at 100 samples per symbol, carrier offset `offset` cycles per sample, AWGN; gaps: [a, b) stretches at 1 % amplitude
    (below the noise gate: they freeze the loop).  Returns (iq, noise threshold)."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, order, n // 100 + 1)
    phases = (np.array([-135, -45, 45, 135]) if order == 4 else np.array([-90, 90]))[sym] * np.pi / 180
    ph = np.repeat(phases, 100)[:n] + 2 * np.pi * offset * np.arange(n)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1) + 0.1 * np.sqrt(0.5) * rng.standard_normal((n, 2))
    for a, b in gaps:
        iq[a:b] *= 0.01
    if dtype == np.float32:
        return iq.astype(np.float32), 0.2
    info = np.iinfo(dtype)
    scale, off = (info.max - info.min) / 2 * 0.7, (info.max + info.min + 1) / 2
    iq = np.clip(np.round(iq * scale + off), info.min, info.max).astype(dtype)
    return iq, (0.0 if np.dtype(dtype).kind == "u" else 0.2 * scale)


def params(order, noise, bandwidth=0.1):
    from urh_amd.pipeline import DemodParams
    return DemodParams("PSK", 2 if order == 4 else 1, noise, 0.0, 1.5 if order == 4 else 1.0, 5, 100, bandwidth, 8, True)


def run_sharded(engines, shards, bounds, n, p, halos, timeout=600):
    """the PSK pass with len(shards) ranks as threads; returns (results, per-rank last_costas, per-rank exception)"""
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    world = len(shards)
    shared = ThreadComm.Shared(world)
    out, recs, err = [None] * world, [None] * world, [None] * world

    def work(r):
        try:
            sp = ShardedPipeline(engines[r], ThreadComm(shared, r))
            out[r] = sp.iq_to_bits(shards[r], p, want_qad=True, pos_base=bounds[r][0], n_total=n, left_raw=halos[r])
            recs[r] = sp.last_costas
        except BaseException as e:          # noqa: BLE001 -- reported by the caller
            err[r] = e
            shared.barrier.abort()          # the other ranks leave their collective instead of waiting for this one
    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), "a rank hangs"
    return out, recs, err


def check(pipe, engines, iq, p, bounds, oracle=None):
    """sharded == single GPU (== oracle); returns the ranks' Costas records"""
    import torch
    from urh_amd.sharding import costas_halo_samples, stitch
    n = iq.shape[0]
    dev = torch.from_numpy(iq).cuda()
    single = pipe.iq_to_bits(dev, p, want_qad=True)
    want = (single.ppseq().copy(),) + tuple(x.copy() for x in single.flat())
    want_qad = single.qad.cpu().numpy().copy()
    if oracle is not None and n <= ORACLE_MAX:
        qad = oracle.afp_demod(iq, p.noise_threshold, "PSK", 4 if p.bits_per_symbol == 2 else 2, p.costas_loop_bandwidth)
        qad[0] = -4.0                                       # the reference leaves it unwritten (np.empty)
        pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, "PSK", p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
        fb = oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)
        assert bits_equal(want_qad, qad) and np.array_equal(want[0], pp)
        assert all(np.array_equal(a, b) for a, b in zip(fb, want[1:]))
    shards = [dev[a:b] for a, b in bounds]
    halos = [None] + [dev[a - costas_halo_samples(p.costas_loop_bandwidth, a):a] for a, _ in bounds[1:]]
    res, recs, err = run_sharded(engines, shards, bounds, n, p, halos)
    assert not any(err), err
    got = stitch(res)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (bounds, k, len(a), len(b))
    got_qad = np.concatenate([r.qad.cpu().numpy() for r in res])
    assert bits_equal(got_qad, want_qad), (bounds, int((got_qad.view(np.uint32) != want_qad.view(np.uint32)).sum()))
    rounds = {rec["rounds"] for rec in recs}
    assert len(rounds) == 1, recs                          # every rank took the same number of rounds
    return recs


def random_cuts(rng, n, world, lo=8):
    cuts = sorted(int(c) * 8 for c in rng.choice(np.arange(lo // 8 + 1, n // 8), size=world - 1, replace=False))
    e = [0] + cuts + [n]
    return [(e[r], e[r + 1]) for r in range(world)]


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_psk_shards_equal_single_gpu(pipe, engines, oracle, order, world):
    from urh_amd.sharding import shard_bounds
    n = 240_000
    iq, noise = psk_capture(n, order, seed=10 * world + order)
    p = params(order, noise)
    recs = check(pipe, engines, iq, p, shard_bounds(n, world), oracle)
    assert recs[0]["rounds"] == 1, recs                   # the loop has locked long before every cut: one exchange
    check(pipe, engines, iq, p, random_cuts(np.random.default_rng(world * 31 + order), n, world, lo=20_000), oracle)


@pytest.mark.parametrize("dtype", [np.float32, np.int8, np.uint8, np.int16, np.uint16])
def test_psk_shards_sample_types(pipe, engines, oracle, dtype):
    from urh_amd.sharding import shard_bounds
    n = 200_000
    iq, noise = psk_capture(n, 4, seed=np.dtype(dtype).itemsize, dtype=dtype, gaps=((90_000, 93_000),))
    p = params(4, noise)
    check(pipe, engines, iq, p, shard_bounds(n, 3), oracle)
    check(pipe, engines, iq, p, [(0, 91_000), (91_000, 150_008), (150_008, n)], oracle)


@pytest.mark.parametrize("bandwidth", [0.01, 0.1, 0.5])
def test_psk_shards_bandwidths(pipe, engines, oracle, bandwidth):
    from urh_amd.sharding import shard_bounds
    n = 300_000
    iq, noise = psk_capture(n, 4, seed=int(bandwidth * 1000), offset=0.002)
    p = params(4, noise, bandwidth)
    check(pipe, engines, iq, p, shard_bounds(n, 3), oracle)
    check(pipe, engines, iq, p, random_cuts(np.random.default_rng(int(bandwidth * 100)), n, 3), oracle)


def test_psk_shards_adversarial_cuts(pipe, engines, oracle):
    """cuts inside a gated stretch longer than the look-back (8192 samples at bandwidth 0.1), a shard that is entirely gated, cuts
    before the loop has locked, a shard shorter than one chunk (4096) and shards shorter than their halo: exact, and the breaks take
    more than one round"""
    n = 300_000
    iq, noise = psk_capture(n, 4, seed=77, gaps=((100_000, 140_000), (200_000, 230_000)))
    p = params(4, noise)
    edges = [0, 200, 3_000, 7_000, 8_000, 60_000, 104_000, 120_000, 136_000, 215_000, n]
    recs = check(pipe, engines, iq, p, [(edges[r], edges[r + 1]) for r in range(len(edges) - 1)], oracle)
    assert recs[0]["rounds"] > 1, recs
    # only the short / early shards: exact whatever the rounds
    edges = [0, 200, 3_000, 7_000, 8_000, n]
    check(pipe, engines, iq, p, [(edges[r], edges[r + 1]) for r in range(len(edges) - 1)], oracle)


def test_psk_config5_eight_threads(pipe, engines):
    """SURVEY 8(d) config 5 at 2^24 samples over 8 ranks: exact, one round, no chunk evaluated serially"""
    import torch
    from urh_amd.sharding import shard_bounds
    from urh_amd.synth import spec_psk_capture
    iq, _ = spec_psk_capture(16, torch.device("cuda", 0))
    host = iq.cpu().numpy()
    del iq
    p = params(4, 0.2)
    recs = check(pipe, engines, host, p, shard_bounds(host.shape[0], 8))
    assert all(r["rounds"] == 1 for r in recs), recs


def test_psk_missing_halo_raises_and_does_not_hang(engines):
    """a rank > 0 without its raw halo (or with too short a one) raises ValueError with the count it needs; the other ranks come
    back instead of waiting for it"""
    import torch
    from urh_amd.sharding import shard_bounds
    n = 60_000
    iq, noise = psk_capture(n, 4, seed=5)
    p = params(4, noise)
    dev = torch.from_numpy(iq).cuda()
    bounds = shard_bounds(n, 3)
    shards = [dev[a:b] for a, b in bounds]
    for halo2 in (None, dev[bounds[2][0] - 100:bounds[2][0]]):
        halos = [None, dev[bounds[1][0] - 8192:bounds[1][0]], halo2]
        _, _, err = run_sharded(engines, shards, bounds, n, p, halos, timeout=120)
        assert isinstance(err[2], ValueError) and "8192" in str(err[2]), err
        assert all(e is not None for e in err[:2]), err     # the others left their collective (broken barrier), none hangs


def test_psk_pipelined_engine_refuses():
    import torch
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import ShardedPipeline, ThreadComm
    iq, noise = psk_capture(20_000, 4, seed=1)
    sp = ShardedPipeline(GpuShardEngine(0, pipelined=True), ThreadComm(ThreadComm.Shared(1), 0))
    with pytest.raises(ValueError, match="pipelined"):
        sp.iq_to_bits(torch.from_numpy(iq).cuda(), params(4, noise))
