"""Seeded PSK captures and the oracle's results for the tests of the PSK batch (tests/test_batch_psk_gpu.py; urh_amd/batch/
iq_to_bits_batch_psk).  The generator follows the recipe of tests/test_costas_shard.py::psk_capture: PSK at 100 samples per symbol with a
carrier offset, AWGN, gated gaps at 1 % amplitude, and the integer sample types with their thresholds."""
import numpy as np

TILE = 64          # samples per tile of k_batch_costas = captures per wavefront


def psk_capture(n, order, seed, dtype=np.float32, gaps=(), offset=0.04):
    """Returns (iq, noise threshold); gaps: [a, b) stretches at 1 % amplitude (below the noise gate: they freeze the loop)"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, order, n // 100 + 1)
    phases = (np.array([-135, -45, 45, 135]) if order == 4 else np.array([-90, 90]))[sym] * np.pi / 180
    ph = np.repeat(phases, 100)[:n] + 2 * np.pi * offset * np.arange(n)
    iq = np.stack([np.cos(ph), np.sin(ph)], 1).reshape(n, 2) + 0.1 * np.sqrt(0.5) * rng.standard_normal((n, 2))
    for a, b in gaps:
        iq[a:b] *= 0.01
    if dtype == np.float32:
        return iq.astype(np.float32), 0.2
    info = np.iinfo(dtype)
    scale, off = (info.max - info.min) / 2 * 0.7, (info.max + info.min + 1) / 2
    iq = np.clip(np.round(iq * scale + off), info.min, info.max).astype(dtype)
    return iq, (0.0 if np.dtype(dtype).kind == "u" else 0.2 * scale)


def params(order, noise, bandwidth=0.1, bps=None, tolerance=5):
    from urh_amd.pipeline import DemodParams
    bps = (2 if order == 4 else 1) if bps is None else bps
    return DemodParams("PSK", bps, noise, 0.0, 1.5 if order == 4 else 1.0, tolerance, 100, bandwidth, 8, False)


def reference(oracle, iq, p):
    """(qad, pulse table, (bits, offsets, pauses, positions, position offsets)) of the oracle, as tests/test_psk_stream.py::reference"""
    qad = oracle.afp_demod(iq, p.noise_threshold, "PSK", 2 ** p.bits_per_symbol, p.costas_loop_bandwidth)
    if len(qad) > 2:
        qad[0] = -4.0                                      # the reference leaves it unwritten (np.empty)
    pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, "PSK", p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
    return qad, np.asarray(pp).reshape(-1, 2), oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)


def same(h, want, qad=None, tag=None, nan_payloads=True):
    """a HostBits and its demodulated signal against reference(): qad as uint32 from index 0, the pulse table, bits, offsets, pauses and the
    derived positions.  nan_payloads=False: where both signals hold a NaN its payload is not compared (edge_inputs.same_bits)"""
    wq, pp, flat = want
    assert h.truncated == 0 and h.rows_needed == len(pp), (tag, h.truncated, h.rows_needed, len(pp))
    if qad is not None:
        got = qad.cpu().numpy()
        assert got.shape == wq.shape, (tag, got.shape, wq.shape)
        if nan_payloads:
            bad = np.nonzero(got.view(np.uint32) != wq.view(np.uint32))[0]
            assert bad.size == 0, (tag, "qad", bad[:5], got[bad[:5]], wq[bad[:5]])
        else:
            import edge_inputs as E
            assert E.same_bits(got, wq).all(), (tag, "qad")
    assert np.array_equal(h.ppseq(), pp), tag
    assert np.array_equal(h.bits(), flat[0]) and np.array_equal(h.msg_off, flat[1]) and np.array_equal(h.pauses, flat[2]), tag
    assert np.array_equal(h.bit_sample_pos(), flat[3]) and np.array_equal(h.pos_offsets(), flat[4]), tag
    for a, b in zip(h.flat(), flat):
        assert np.array_equal(a, b), tag


def gapped(n, order, seed, dtype=np.float32):
    """a capture of n samples with a gated stretch in its second third (none where it is too short for one)"""
    gaps = ((n // 3, n // 3 + n // 7 + 3),) if n >= 100 else ()
    return psk_capture(n, order, seed, dtype=dtype, gaps=gaps)


def to_dev(pipe, iq):
    import torch
    a = np.ascontiguousarray(iq)
    if a.dtype == np.uint16 and hasattr(torch, "uint16"):
        return torch.from_numpy(a.view(np.int16)).to(pipe.device).view(torch.uint16)
    return torch.from_numpy(a).to(pipe.device)
