"""A numpy model of the message records of a BATCH of captures (include/urhgpu.h "a batch of captures: message records per capture";
urh_amd/csrc/batch_records.hip), written from its semantics on top of tests/model_msg_records.py and independent of urh_amd:
    directory()   the exclusive prefix of the captures' message counts
    sweep()       the three positions a record needs, derived from a capture's pulse-table rows in ONE sweep with the walk's control flow --
                  the leading pause only seeds total_samples, a long pause closes a message or drops what was gathered, the trailing
                  message -- the message's length and pause known before its rows are swept
    records()     the records of the whole batch, each window Python's slice of its OWN capture (clip=False: of the rest of the buffer, the
                  bug the clipping guards against)
"""
import numpy as np

import model_msg_records as mm

RECORD_DTYPE = mm.RECORD_DTYPE


def directory(n_msg):
    """rec_dir[c] = records of the captures before c; rec_dir[K] = all of them"""
    return np.concatenate([[0], np.cumsum(np.asarray(n_msg, dtype=np.int64))]).astype(np.int64)


def n_pad_of(ln, pause, mod, sps, divisor):
    if mod == "ASK" and divisor > 1 and ln >= 0:
        missing = (divisor - ln % divisor) % divisor
        if missing > 0 and pause >= sps * missing:
            return missing
    return 0


def sweep(rows, msg_off, pauses, mod, sps, bps, pause_threshold, divisor):
    """rows: the pulse table (P, 2) = [state, length] as grab_pulse_lens gives it (PAUSE = -1); msg_off / pauses: the digitisation's.
    Returns per message (first_pos, entry np - 2, mid_pos, n_pad, ok)."""
    spb = int(sps / bps)
    n_msg = len(pauses)
    out = []
    ts = nb = m = 0
    data = have_t = False
    first = pos_t = last_bit = 0
    state = {}

    def load():
        state.clear()
        if m < n_msg:
            ln = int(msg_off[m + 1] - msg_off[m])
            pad = n_pad_of(ln, int(pauses[m]), mod, sps, divisor)
            k = (ln + pad) // 2
            state.update(ln=ln, pad=pad, k=k, t=min(k, ln - 1))

    def close(closed, a):
        ln, pad, k = state.get("ln", -1), state.get("pad", 0), state.get("k", 0)
        ok = m < n_msg and ln >= 1 and nb == ln and have_t
        mid = pos_t
        if closed:
            entry = a                                      # np = ln + 2: entry ln is the closing pause's start
            if k >= ln:
                mid = a + (k - ln) * sps
        else:
            entry = last_bit                               # np = ln + 1: entry ln - 1 is the last bit
            if k > ln - 1:
                mid = pos_t + (k - (ln - 1)) * sps
        out.append((first, entry, mid, pad, ok))

    load()
    for r, (s, ln_row) in enumerate(np.asarray(rows, dtype=np.int64).reshape(-1, 2).tolist()):
        a = abs(ln_row)
        q = a // sps
        nsym = -q if ln_row < 0 else q + (1 if 2 * (a - q * sps) > sps else 0)
        if r == 0 and s == -1:
            ts += ln_row
            continue
        if s == -1 and not (nsym <= pause_threshold or pause_threshold == 0):
            if data:
                close(True, ts)
                m += 1
                load()
                data = False
            nb, have_t = 0, False
            ts += ln_row
            continue
        k_bits = nsym * bps
        if k_bits > 0:
            if nb == 0:
                first = ts
            t = state.get("t", -1)
            if not have_t and nb <= t < nb + k_bits:
                pos_t, have_t = ts + (t - nb) * spb, True
            nb += k_bits
            last_bit = ts + (k_bits - 1) * spb
        if s != -1 and not data and nsym > 0:
            data = True
        ts += ln_row
    if data:
        close(False, ts)
    return out


def records(iq_cat, starts, tables, mod, sps, bps, pause_threshold, divisor, clip=True):
    """tables: per capture (rows, msg_off, pauses).  Returns (rec_dir, records of the batch back to back, the capture of each record)."""
    iq_cat = np.asarray(iq_cat)
    norm = mm.norm_of(iq_cat.dtype)
    rec_dir = directory([len(t[2]) for t in tables])
    rec = np.zeros(int(rec_dir[-1]), RECORD_DTYPE)
    cap = np.zeros(int(rec_dir[-1]), np.int32)
    for c, (rows, msg_off, pauses) in enumerate(tables):
        s0, s1 = int(starts[c]), int(starts[c + 1])
        own = iq_cat[s0:s1] if clip else iq_cat[s0:]      # (Python's slice of the capture -- or, wrongly, of everything behind its start)
        for m, (first, _, mid, pad, ok) in enumerate(sweep(rows, msg_off, pauses, mod, sps, bps, pause_threshold, divisor)):
            window = own[mid:mid + sps]
            with np.errstate(invalid="ignore", divide="ignore"):
                rec[rec_dir[c] + m] = (mm.mean64(mm.magnitudes(window) / norm), first, mid, pad, 1 if ok else 0)
            cap[rec_dir[c] + m] = c
    return rec_dir, rec, cap
