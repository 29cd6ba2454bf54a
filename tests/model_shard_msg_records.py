"""Executable model (numpy, CPU tensors) of the engine methods behind ShardedPipeline.message_records (urh_amd/shard_engine.py:
records_summary, records_lookup, records_window_part, records_finish), written from their definitions in include/urhgpu.h ("message records
of a sharded capture") on top of tests/model_msg_records.py (mean64, magnitudes, norm_of and the padding rule).  The "result" of a pass is
the piece tests/model_shard.py's engine returns: dict(rows, bits, msg_end, pauses, pos, pos_end) with LOCAL end offsets and global
positions; the shard is the raw IQ as a numpy array.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import model_msg_records as mm

SUMMARY_WORDS, FIRST_WORDS = 10, 8


def n_pad_of(L, pause, sps, divisor):
    """the padding rule of model_msg_records.records"""
    if divisor > 1:
        missing = (divisor - L % divisor) % divisor
        if missing > 0 and pause >= sps * missing:
            return missing
    return 0


def py_window(mid, sps, n):
    """iq[mid:mid + sps] on n samples as (begin, count)"""
    idx = range(n)[mid:mid + sps]
    return (idx.start, len(idx)) if len(idx) else (min(max(mid, 0), n), 0)


class ModelRecordsEngine:
    """the four records methods on one rank's piece; `held` False models a rank whose pass exceeded a capacity"""

    def __init__(self, held=True):
        self.held = held
        self.exchanged = []                 # the windows this rank was asked to contribute to: (lo, w)

    def records_summary(self, iq_local, piece, pos_base):
        n_msg, n_bits, n_pos = len(piece["pauses"]), len(piece["bits"]), len(piece["pos"])
        w = np.zeros(SUMMARY_WORDS, np.int64)
        w[0], w[1], w[2] = pos_base, len(iq_local), n_msg
        w[3] = piece["msg_end"][0] if n_msg else n_bits
        w[4] = piece["pos_end"][0] if n_msg else n_pos
        w[5] = n_bits - piece["msg_end"][-1] if n_msg else 0
        w[6] = n_pos - piece["pos_end"][-1] if n_msg else 0
        w[7] = piece["pauses"][0] if n_msg else 0
        w[8] = 1 if self.held else 0
        w[9] = n_pos
        return torch.from_numpy(w)

    def records_lookup(self, piece, index):
        pos = np.asarray(piece["pos"], np.int64)
        out = np.zeros(len(index), np.int64)
        for i, at in enumerate(np.asarray(index).tolist()):
            if 0 <= at < len(pos):
                out[i] = pos[at]
        return torch.from_numpy(out)

    def records_window_part(self, iq_local, pos_base, spans, w_max):
        iq = np.ascontiguousarray(iq_local)
        raw = iq.view(np.uint8).reshape(len(iq), -1)
        part = np.zeros((len(spans), int(w_max), raw.shape[1]), np.uint8)
        for j, (lo, w) in enumerate(spans):
            self.exchanged.append((lo, w))
            a, b = max(lo, pos_base), min(lo + w, pos_base + len(iq))
            if b > a:
                part[j, a - lo:b - lo] = raw[a - pos_base:b - pos_base]
        return torch.from_numpy(part)

    def records_finish(self, iq_local, piece, pos_base, n_total, p, divisor, first, window):
        iq = np.ascontiguousarray(iq_local)
        sps, norm = int(p.samples_per_symbol), mm.norm_of(iq.dtype)
        divisor = int(divisor) if p.modulation_type == "ASK" else 1
        n_msg = len(piece["pauses"])
        msg_off = np.concatenate([[0], np.asarray(piece["msg_end"], np.int64)])
        pos_off = np.concatenate([[0], np.asarray(piece["pos_end"], np.int64)])
        pos = np.asarray(piece["pos"], np.int64)
        out = np.zeros(n_msg, mm.RECORD_DTYPE)
        for m in range(n_msg):
            if m == 0:
                assert int(first[0]) == 1
                n_pad, ok = int(first[3]), self.held and int(first[6]) == 1
                first_pos, mid = (int(first[4]), int(first[5])) if ok else (0, 0)
            else:
                L, ent = int(msg_off[m + 1] - msg_off[m]), pos[pos_off[m]:pos_off[m + 1]]
                n_pad = n_pad_of(L, int(piece["pauses"][m]), sps, divisor)
                k = (L + n_pad) // 2
                in_pad = n_pad > 0 and k > len(ent) - 2
                rel = len(ent) - 2 if in_pad else k
                ok = self.held and len(ent) >= 1 and 0 <= rel < len(ent)
                first_pos, mid = (int(ent[0]), int(ent[rel]) + ((k - rel) * sps if in_pad else 0)) if ok else (0, 0)
            if not ok:
                out[m] = (np.nan, 0, 0, n_pad, 0)
                continue
            lo, w = py_window(mid, sps, int(n_total))
            if m == 0 and int(first[7]) == 1:
                samples = np.ascontiguousarray(window.numpy()).reshape(-1).view(iq.dtype).reshape(-1, 2)[:w]
                assert len(samples) == w
            elif w > 0 and (lo < pos_base or lo + w > pos_base + len(iq)):
                out[m] = (np.nan, first_pos, mid, n_pad, -2)                # nothing outside the shard is read
                continue
            else:
                samples = iq[lo - pos_base:lo - pos_base + w]
            with np.errstate(invalid="ignore", divide="ignore"):
                out[m] = (mm.mean64(mm.magnitudes(samples) / norm), first_pos, mid, n_pad, 1)
        return out


def pass_and_records_engine(held=True, **kw):
    """one engine with the pass of tests/model_shard.py (on the demodulated signal) and the records methods above (on the raw IQ)"""
    import model_shard

    class Engine(model_shard.ModelShardEngine, ModelRecordsEngine):
        def __init__(self):
            model_shard.ModelShardEngine.__init__(self, **kw)
            ModelRecordsEngine.__init__(self, held)
    return Engine()
