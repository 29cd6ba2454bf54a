"""Tiles of the row table are the chunks ONE tail wavefront owns (pulse_table.hip: kTileChunks = kTailCPW = 4 consecutive chunks), not
single chunks: the row kernel accumulates a tile's aggregate across its chunks, the tile scan and the expansion work on a quarter of the
tiles.  Whatever the grouping, every route -- staged stream passes, the latency setting, uploads, one-shot iq_to_bits, the table passes
of sharded captures (one chunk per tile still) -- returns the rows, bits, message offsets, pauses, positions and the demodulated signal
the reference computes (oracle = the C restatement pinned on the reference, tests/test_oracle.py), element for element.

The captures run under the chunk plan of a 1 GiB capture (urhgpu_test_force_tiles_per_chunk(4): chunks of 8192 samples, tiles of 32768)
at sizes where grouping can go wrong: 1 .. 11 chunks (no tile, one partly filled tile, whole tiles, whole tiles and a remainder of one to
three chunks), with and without a partial last chunk; dense pulse tables (8 - 10 samples per symbol, tolerance 0 and 1: more than 64
records in a chunk, more than 256 rows in a tile); rows of more than 4096 bits inside a tile, as a tile's first row and as the table's last
row; long pauses on chunk and tile boundaries; one long pause; no accepted run at all."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = 8192                  # samples per chunk under the forced plan
TILE = 4 * CH              # samples per tile
N_MAX = 12 * CH


@pytest.fixture()
def gib_plan():
    from urh_amd import _lib
    lib = _lib.load()
    lib.urhgpu_test_force_tiles_per_chunk(4)
    yield
    lib.urhgpu_test_force_tiles_per_chunk(0)


def _capture(n, sps, seed, noise=0.03, tones=(), pauses=(), flip_every=0):
    """2-FSK (continuous phase, +-20 kHz at 1 MS/s) of random symbols; tones: [a, b) of ONE frequency (a single long row); pauses: [a, b)
    silent; flip_every: the frequency alternates every that many samples instead (runs no longer than a tolerance above it)"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n // sps + 1)
    f = np.repeat(np.where(bits == 1, 20e3, -20e3), sps)[:n]
    if flip_every:
        f = np.where((np.arange(n) // flip_every) % 2 == 1, 20e3, -20e3)
    for a, b in tones:
        f[a:b] = 20e3
    phase = np.cumsum(2 * np.pi * f / 1e6)
    iq = np.stack([np.cos(phase), np.sin(phase)], axis=1)
    for a, b in pauses:
        iq[max(a, 0):b] = 0
    return (iq + noise * rng.standard_normal((n, 2))).astype(np.float32)


SIZES = [1 * CH, 2 * CH, 3 * CH, 4 * CH, 5 * CH, 7 * CH, 9 * CH, 10 * CH, 11 * CH,       # 1, 2, 3, 4, 5, 7 and 4k + 1 .. 4k + 3 chunks
         2 * CH + 3001, 4 * CH + 1, 8 * CH + 5000, 11 * CH + 777]                        # a partial last chunk behind 2, 4, 8, 11 chunks


def _dense(sps):
    return [(f"dense {n}", _capture(n, sps, 1000 + i)) for i, n in enumerate(SIZES)]


def _boundary_pauses(sps, seed):
    """long pauses (more than 8 symbols) that end on, begin on and straddle every chunk boundary -- every fourth one a tile boundary"""
    lp = 40 * sps
    pauses = []
    for k, b in enumerate(range(CH, N_MAX - CH + 1, CH)):
        pauses.append([(b - lp, b), (b, b + lp), (b - lp // 2, b + lp // 2), (b - lp - 1, b + 1)][k % 4])
    pauses += [(TILE - lp, TILE), (2 * TILE, 2 * TILE + lp)][seed % 2:seed % 2 + 1]
    return _capture(N_MAX - (seed % 2) * 1234, sps, seed, pauses=pauses)


def _huge_rows(sps, bps, seed):
    """rows of more than 4096 bits (kHugeBits): tones of 4200 / bps symbols"""
    ln = 4200 // bps * sps
    assert ln < TILE - 4000
    return [("huge inside a tile", _capture(N_MAX, sps, seed, tones=[(TILE + 2000, TILE + 2000 + ln)])),
            ("huge as a tile's first row", _capture(N_MAX, sps, seed + 1, tones=[(2 * TILE - 3000, 2 * TILE - 3000 + ln)])),
            ("huge as the table's last row", _capture(5 * CH + 123, sps, seed + 2, tones=[(5 * CH + 123 - ln, 5 * CH + 123)])),
            ("huge last row, whole tiles", _capture(8 * CH, sps, seed + 3, tones=[(8 * CH - ln - 50, 8 * CH)])),
            ("huge rows and a pause", _capture(N_MAX, sps, seed + 4, tones=[(100, 100 + ln), (TILE + CH - 10, TILE + CH - 10 + ln)],
                                               pauses=[(3 * TILE - 700, 3 * TILE + 900)]))]


def _flat(n_list):
    rng = np.random.default_rng(5)
    out = [(f"one long pause {n}", (0.02 * rng.standard_normal((n, 2))).astype(np.float32)) for n in n_list]
    # the frequency flips every 3 samples, tolerance 5: no run is ever accepted, the table is its last row alone
    out += [(f"no accepted run {n}", _capture(n, 10, 77, noise=0.0, flip_every=3)) for n in n_list]
    return out


def _params(name, want_pos=True):
    from urh_amd.pipeline import DemodParams
    return {
        "dense_tol0": DemodParams("FSK", 1, 0.1, 0.0, 1.0, 0, 9, 0.1, 8, want_pos),
        "dense_tol1": DemodParams("FSK", 1, 0.1, 0.0, 1.0, 1, 8, 0.1, 8, want_pos),
        "fsk4": DemodParams("FSK", 2, 0.1, 0.0, 0.03, 1, 10, 0.1, 8, want_pos),
        "huge": DemodParams("FSK", 1, 0.1, 0.0, 1.0, 2, 4, 0.1, 8, want_pos),
        "huge_fsk4": DemodParams("FSK", 2, 0.1, 0.0, 0.03, 2, 8, 0.1, 8, want_pos),
        "flat": DemodParams("FSK", 1, 0.1, 0.0, 1.0, 5, 10, 0.1, 8, want_pos),
    }[name]


def _build(name):
    if name == "dense_tol0":
        return _dense(9) + [("pauses on boundaries a", _boundary_pauses(9, 2)), ("pauses on boundaries b", _boundary_pauses(9, 3))]
    if name == "dense_tol1":
        return _dense(8) + [("pauses on boundaries a", _boundary_pauses(8, 4)), ("pauses on boundaries b", _boundary_pauses(8, 5))]
    if name == "fsk4":
        return _dense(10)[::2] + [("pauses on boundaries a", _boundary_pauses(10, 6)), ("pauses on boundaries b", _boundary_pauses(10, 7))]
    if name == "huge":
        return _huge_rows(4, 1, 31)
    if name == "huge_fsk4":
        return _huge_rows(8, 2, 41)   # two bits per symbol
    return _flat([CH, 3 * CH, 4 * CH + 1, 9 * CH, N_MAX])


CONFIGS = ["dense_tol0", "dense_tol1", "fsk4", "huge", "huge_fsk4", "flat"]
_cache = {}


def _cases(oracle, name):
    """the captures of a configuration and what the oracle computes for them: (tag, iq, qad, (rows, bits, msg_off, pauses, pos, pos_off)),
    computed once and shared by every route"""
    if name not in _cache:
        p = _params(name)
        caps = _build(name)
        out = []
        for tag, iq in caps:
            qad = oracle.afp_demod(iq, p.noise_threshold, "FSK", 2 ** p.bits_per_symbol)
            pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, "FSK", p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
            flat = tuple(oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold))
            for a in (qad, pp) + flat:
                a.setflags(write=False)
            out.append((tag, iq, qad, (pp,) + flat))
        _cache[name] = out
    return _cache[name]


def test_the_cases_are_what_they_claim(oracle):
    """dense tables have more than 64 records per chunk and more than 256 rows per tile; the huge rows hold more than 4096 bits; the flat
    captures are one pause row"""
    for name in ("dense_tol0", "dense_tol1"):
        for tag, iq, _, ref in _cases(oracle, name):
            if tag.startswith("dense"):
                assert len(ref[0]) > 65 * (-(-len(iq) // CH)) and (len(iq) < TILE or len(ref[0]) > 257 * (len(iq) // TILE)), (name, tag, len(ref[0]))
    for name, sps, bps in (("huge", 4, 1), ("huge_fsk4", 8, 2)):
        for tag, iq, _, ref in _cases(oracle, name):
            if tag.startswith("huge"):
                assert (ref[0][:, 1] // sps * bps).max() > 4096, (name, tag)
        tag, iq, _, ref = _cases(oracle, name)[2]
        assert ref[0][-1, 1] // sps * bps > 4096, (name, tag)
    for tag, iq, _, ref in _cases(oracle, "flat"):
        assert len(ref[0]) == 1, (tag, len(ref[0]))


def _assert_equal(got, ref, tag, want_pos=True):
    names = ("rows", "bits", "msg_off", "pauses", "pos", "pos_off")
    for k, (name, g, e) in enumerate(zip(names, got, ref)):
        if k >= 4 and not want_pos:
            break
        if not np.array_equal(g, e):
            g, e = np.asarray(g), np.asarray(e)
            m = min(len(g), len(e))
            first = int(np.argmax(g[:m].reshape(m, -1) != e[:m].reshape(m, -1))) if m else -1
            raise AssertionError(f"{tag}: {name} differs (got {g.shape}, expected {e.shape}, first difference near flat index {first})")


def _host(r):
    r.check()
    return (r.ppseq(), r.bits(), r.msg_off.copy(), r.pauses.copy(), r.bit_sample_pos(), r.pos_offsets())


def _qad_of(pipe, r, n):
    from urh_amd import _lib
    q = np.empty(n, np.float32)
    _lib.check(_lib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(r.d_qad_ptr), q.ctypes.data_as(C.c_void_p), n * 4))
    return q


def _cap_rows(p):
    return N_MAX // (p.tolerance + 1) + 2


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_staged_stream_equals_oracle(oracle, gib_plan, name, want_pos):
    """pushes of different captures back to back through one stream (the default policy: staged or direct passes, pack + copy for
    captures with a partial last chunk)"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    cases = _cases(oracle, name)
    assert len(cases) >= 4
    p = _params(name, want_pos)
    pipe = DevicePipeline(0, pipelined=True)
    st = pipe.stream(N_MAX, p, want_qad=True, want_pos=want_pos, cap_rows=_cap_rows(p))
    dev = [torch.from_numpy(iq).cuda() for _, iq, _, _ in cases]
    got = {}
    for d in dev:
        r = st.push(d)
        if r is not None:
            got[r.seq] = _host(r)
    for r in st.flush():
        got[r.seq] = _host(r)
    st.close()
    for i, (tag, iq, _, ref) in enumerate(cases):
        _assert_equal(got[i], ref, f"{name}, {tag}")      # (positions not shipped are derived from the shipped pulse table: the same)


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_latency_setting_equals_oracle(oracle, gib_plan, name, want_pos):
    """stream_latency = 1: every capture pushed and flushed on its own (the segmented tail where the capture is long enough to be cut),
    the demodulated signal of every pass read back"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    cases = _cases(oracle, name)
    p = _params(name, want_pos)
    pipe = DevicePipeline(0, pipelined=True)
    st = pipe.stream(N_MAX, p, want_qad=True, want_pos=want_pos, cap_rows=_cap_rows(p), latency=True)
    for tag, iq, qad, ref in cases:
        assert st.push(torch.from_numpy(iq).cuda()) is None
        (r,) = st.flush()
        _assert_equal(_host(r), ref, f"{name}, {tag}")
        assert np.array_equal(_qad_of(pipe, r, len(iq)).view(np.uint32), qad.view(np.uint32)), f"{name}, {tag}: qad"
    st.close()
    pipe.ctx.set_tuning("stream_latency", 0)


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_upload_equals_oracle(oracle, gib_plan, name, want_pos):
    """urhgpu_stream_push_upload: the capture starts in pinned host memory"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    cases = _cases(oracle, name)
    p = _params(name, want_pos)
    pipe = DevicePipeline(0, pipelined=True)
    st = pipe.stream(N_MAX, p, want_qad=False, want_pos=want_pos, cap_rows=_cap_rows(p))
    host = [torch.from_numpy(iq).pin_memory() for _, iq, _, _ in cases]
    dev = [torch.zeros_like(h, device="cuda") for h in host]
    got = {}
    for h, d in zip(host, dev):
        r = st.push_upload(h, d)
        if r is not None:
            got[r.seq] = _host(r)
    for r in st.flush():
        got[r.seq] = _host(r)
    st.close()
    torch.cuda.synchronize()
    for i, (tag, iq, _, ref) in enumerate(cases):
        assert np.array_equal(dev[i].cpu().numpy().view(np.uint32), iq.view(np.uint32)), f"{name}, {tag}: the device buffer does not hold the capture"
        _assert_equal(got[i], ref, f"{name}, {tag}")


@pytest.mark.parametrize("want_pos", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_one_shot_equals_oracle(oracle, gib_plan, name, want_pos):
    """iq_to_bits, one capture per call (launch_tile_rows / launch_tile_bits over the whole capture), the demodulated signal included"""
    import torch
    from urh_amd.pipeline import DevicePipeline
    p = _params(name, want_pos)
    pipe = DevicePipeline(0)
    for tag, iq, qad, ref in _cases(oracle, name):
        res = pipe.iq_to_bits(torch.from_numpy(iq).cuda(), p, want_qad=True, cap_rows=_cap_rows(p))
        _assert_equal((res.ppseq(),) + tuple(res.flat()), ref, f"{name}, {tag}", want_pos)
        assert np.array_equal(res.qad.cpu().numpy().view(np.uint32), qad.view(np.uint32)), f"{name}, {tag}: qad"


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_equals_single_gpu_and_oracle(oracle, gib_plan, world):
    """2 and 3 simulated ranks (threads, one context each) on this GPU: the table pass of every rank -- the other shards' summaries around
    its own chunks, one chunk per tile -- stitched together equals the single-GPU pass (four chunks per tile) and the oracle; the cuts
    fall inside a dense stretch, inside a long pause and inside a row of more than 4096 bits"""
    import torch
    from test_sharding import run_threads
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import shard_bounds, stitch
    n = 36 * CH + 4321                                    # about 3 * 10^5 samples
    sps, tol = 8, 1
    ln = 4200 * sps
    tone = (n // 2 - ln // 2, n // 2 + ln // 2) if world == 2 else (n // 3 - 5000, n // 3 - 5000 + ln)
    iq = _capture(n, sps, 90 + world, tones=[tone], pauses=[(5 * CH - 300, 5 * CH + 400), (2 * n // 3 - 2000, 2 * n // 3 + 2000), (n - 9000, n - 8000)])
    p = DemodParams("FSK", 1, 0.1, 0.0, 1.0, tol, sps, 0.1, 8, True)
    qad = oracle.afp_demod(iq, 0.1, "FSK", 2)
    pp = oracle.grab_pulse_lens(qad, 0.0, tol, "FSK", sps, 1, 1.0)
    ref = (pp,) + tuple(oracle.ppseq_to_bits_flat(pp, sps, 1, True, 8))
    assert (pp[:, 1] // sps).max() > 4096
    dev_iq = torch.from_numpy(iq).cuda()
    single = DevicePipeline(0).iq_to_bits(dev_iq, p, want_qad=True, cap_rows=n // 2 + 2)
    _assert_equal((single.ppseq(),) + tuple(single.flat()), ref, "single GPU")
    assert np.array_equal(single.qad.cpu().numpy().view(np.uint32), qad.view(np.uint32))
    rng = np.random.default_rng(world)
    cuts = [0] + sorted(int(c) * 8 for c in rng.choice(np.arange(1, n // 8), size=world - 1, replace=False)) + [n]
    for bounds in (shard_bounds(n, world), [(cuts[r], cuts[r + 1]) for r in range(world)]):
        shards = [dev_iq[a:b] for a, b in bounds]
        res = run_threads(world, lambda r: GpuShardEngine(0), shards, bounds, n, p, None)
        _assert_equal(stitch(res), ref, f"{world} ranks, bounds {bounds}")
        got_qad = np.concatenate([r.qad.cpu().numpy() for r in res])
        assert np.array_equal(got_qad.view(np.uint32), qad.view(np.uint32)), f"{world} ranks, bounds {bounds}: qad"
