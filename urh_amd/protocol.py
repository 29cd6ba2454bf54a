"""Device-resident counterpart of ProtocolAnalyzer.get_protocol_from_signal
(/root/reference/src/urh/signalprocessing/ProtocolAnalyzer.py:227-321): the O(N) work (demodulation, pulse table, bit
expansion) is one urhgpu_iq_to_bits_dev pass; what remains per message -- padding ASK messages to a multiple of
message_length_divisor (:289-321), the RSSI over one symbol at the middle bit (:267-269), the first bit's position for the
timestamp (:270-272) -- is queued behind the pass as one record per message (include/urhgpu.h: urhgpu_msg_record), while the
capture is still in device memory, and applied here with whole-array operations.  messages_from_bits keeps the host route for
bits that are already on the host.
"""
import array
from dataclasses import dataclass

import numpy as np

# struct urhgpu_msg_record (include/urhgpu.h)
RECORD_DTYPE = np.dtype([("rssi", "<f8"), ("first_pos", "<i8"), ("mid_pos", "<i8"), ("n_pad", "<i4"), ("flag", "<i4")])


@dataclass
class MessageData:
    """The fields ProtocolAnalyzer hands to urh's Message constructor (:273-283)."""
    plain_bits: array.array          # array('B')
    pause: int
    bit_sample_pos: array.array      # array('L')
    rssi: float
    timestamp: float
    samples_per_symbol: int
    bits_per_symbol: int

    @property
    def plain_bits_str(self):
        return "".join(map(str, self.plain_bits))


def _min_max_for_dtype(dtype):
    """IQArray.min_max_for_dtype (src/urh/signalprocessing/IQArray.py:246-250)"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f" or dtype.kind == "c":
        return -1, 1
    return np.iinfo(dtype).min, np.iinfo(dtype).max


def padding_counts(n_bits, pauses, samples_per_symbol, divisor):
    """Zero bits every message borrows from the pause that follows it so that its length becomes a multiple of `divisor`
    (ProtocolAnalyzer.py:303-307): the bits missing to the next multiple, where the pause holds that many symbols, else 0.
    n_bits, pauses: one entry per message."""
    n_bits = np.asarray(n_bits, dtype=np.int64)
    pauses = np.asarray(pauses, dtype=np.int64)
    divisor = int(divisor)
    if divisor <= 1:
        return np.zeros(len(n_bits), np.int64)
    missing = (divisor - n_bits % divisor) % divisor
    return np.where((missing > 0) & (pauses >= int(samples_per_symbol) * missing), missing, 0)


def apply_padding(bits, msg_off, pauses, pos, pos_off, n_pad, samples_per_symbol):
    """The flat outputs of a pass (bits, msg_off, pauses, pos, pos_off as BitsResult.flat() gives them) with message m extended by
    n_pad[m] zero bits: the bits are appended, the pause shrinks by n_pad * samples_per_symbol, and of the message's positions the last
    one is replaced and n_pad more follow: .., A, E become .., A, A + sps, .., A + n_pad * sps, A + n_pad * sps + the new pause (A: the
    start of the closing pause -- or, for a trailing message whose short pause is borrowed from, its last bit's position).
    Whole-array operations; returns new arrays."""
    sps = int(samples_per_symbol)
    n_pad = np.asarray(n_pad, dtype=np.int64)
    msg_off, pos_off = np.asarray(msg_off, dtype=np.int64), np.asarray(pos_off, dtype=np.int64)
    pauses, pos, bits = np.asarray(pauses, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(bits, dtype=np.uint8)
    if not n_pad.any():
        return bits, msg_off, pauses, pos, pos_off
    length, n_entries = np.diff(msg_off), np.diff(pos_off)
    pos_pad = np.where(n_entries >= 2, n_pad, 0)                         # (a message without two positions has none extended)
    shift, pos_shift = np.concatenate([[0], np.cumsum(n_pad)]), np.concatenate([[0], np.cumsum(pos_pad)])      # entries inserted in front of each message
    new_off, new_pos_off = msg_off + shift, pos_off + pos_shift
    new_bits = np.zeros(int(new_off[-1]), np.uint8)
    new_bits[np.arange(len(bits)) + np.repeat(shift[:-1], length)] = bits
    new_pauses = pauses - n_pad * sps
    new_pos = np.zeros(int(new_pos_off[-1]), np.int64)
    new_pos[np.arange(len(pos)) + np.repeat(pos_shift[:-1], n_entries)] = pos    # (a padded message's last entry lands on A + sps's place: overwritten below)
    m = np.nonzero(pos_pad)[0]
    count = pos_pad[m]
    start = pos[pos_off[m] + n_entries[m] - 2]                               # A
    first = new_pos_off[m] + n_entries[m] - 1                                # where A + sps goes
    step = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
    new_pos[np.repeat(first, count) + step] = np.repeat(start, count) + (step + 1) * sps
    new_pos[first + count] = start + count * sps + new_pauses[m]
    return new_bits, new_off, new_pauses, new_pos, new_pos_off


def ensure_message_length_multiple(bit_data, samples_per_symbol, pauses, bit_sample_pos, divisor):
    """ASK messages borrow zero bits from the pause that follows them so that their length becomes a multiple of `divisor`
    (what ProtocolAnalyzer.__ensure_message_length_multiple does, :289-321), in place on the reference-shaped lists:
    padding_counts decides, apply_padding extends."""
    n_msg = len(bit_data)
    n_pad = padding_counts([len(b) for b in bit_data], list(pauses), samples_per_symbol, divisor)
    if n_msg == 0 or not n_pad.any() or len(bit_sample_pos) != n_msg:
        for i in np.nonzero(n_pad)[0].tolist():                                 # (no positions to extend: bits and pauses alone)
            bit_data[i].extend([0] * int(n_pad[i]))
            pauses[i] = pauses[i] - int(n_pad[i]) * int(samples_per_symbol)
        return
    msg_off = np.concatenate([[0], np.cumsum([len(b) for b in bit_data])])
    pos_off = np.concatenate([[0], np.cumsum([len(q) for q in bit_sample_pos])])
    flat_pos = np.concatenate([np.asarray(q, dtype=np.int64) for q in bit_sample_pos])
    _, _, new_pauses, new_pos, new_pos_off = apply_padding(np.zeros(int(msg_off[-1]), np.uint8), msg_off, pauses, flat_pos, pos_off, n_pad,
                                                           samples_per_symbol)
    for i in np.nonzero(n_pad)[0].tolist():
        bit_data[i].extend([0] * int(n_pad[i]))
        pauses[i] = int(new_pauses[i])
        bit_sample_pos[i] = array.array("L", new_pos[new_pos_off[i]:new_pos_off[i + 1]].tolist())


def messages_from_records(flat, records, p, sample_rate=1e6, timestamp=0.0):
    """The list of MessageData from a pass's flat outputs (bits, msg_off, pauses, pos, pos_off) and its records
    (RECORD_DTYPE, one per message): padding applied on whole arrays, RSSI and first position taken from the records."""
    sps, bps = int(p.samples_per_symbol), int(p.bits_per_symbol)
    bits, off, pauses, pos, poff = apply_padding(*flat, records["n_pad"], sps)
    out = []
    for i in range(len(pauses)):
        out.append(MessageData(array.array("B", bits[off[i]:off[i + 1]].tobytes()), int(pauses[i]),
                               array.array("L", pos[poff[i]:poff[i + 1]].tolist()), float(records["rssi"][i]),
                               timestamp + int(records["first_pos"][i]) / sample_rate, sps, bps))
    return out


def get_protocol_from_signal_dev(pipe, iq, p, message_length_divisor=1, sample_rate=1e6, timestamp=0.0):
    """iq: capture on the GPU ((N, 2) tensor of a supported dtype or complex64 (N,)); p: pipeline.DemodParams.
    Returns the list of MessageData the reference would build its Message objects from: one pass with its records queued
    behind it, one hand-out."""
    torch = pipe.torch
    if iq.dtype == torch.complex64:
        iq = torch.view_as_real(iq)
    res = pipe.iq_to_bits_checked(iq, p, want_qad=True, msg_records=True, message_length_divisor=message_length_divisor)
    return res.message_data(sample_rate, timestamp)


def get_protocols_from_signals_dev(pipe, captures, p, message_length_divisor=1, sample_rate=1e6, timestamps=None, auto_noise=False, auto_center=False,
                                   center_max_size=None, cap_rows=None, long_from=None, dc_correction=False):
    """get_protocol_from_signal_dev for a recording session: captures as DevicePipeline.iq_to_bits_batch takes them (a list of numpy arrays
    or device tensors, or (iq_cat, starts)), one parameter set for all.  One batch with its records queued behind it
    (DevicePipeline.iq_to_bits_batch_records); a capture whose pulse table outgrew its capacity is run once more with the rows it needs.
    timestamps: one per capture, default 0.0.  Returns a list of MessageData lists, one per capture in the order given.
    PSK parameters take DevicePipeline.iq_to_bits_batch_psk with the same options.
    dc_correction: every capture minus its own means, corrected on the device in front of the batch (DevicePipeline.iq_to_bits_batch_dc, for
    every modulation a batch takes).
    p may also be a sequence of K DemodParams, one per capture -- what batch.params_from_estimates makes of DevicePipeline.estimate_batch's
    result: the ASK and FSK captures then go through ONE DevicePipeline.iq_to_bits_batch_each (behind dc_correct_batch with dc_correction),
    whatever the number of different parameter sets; PSK captures are split off and run through iq_to_bits_batch_psk ONCE PER DISTINCT PSK
    PARAMETER SET (a Costas loop has no per-capture table); auto_center is refused (estimated parameters carry a center).  The results come
    back in the order given."""
    from .batch import is_psk
    if not hasattr(p, "modulation_type"):
        return _protocols_each(pipe, captures, list(p), message_length_divisor, sample_rate, timestamps, auto_noise, auto_center, cap_rows, long_from,
                               dc_correction)
    if dc_correction:
        res = pipe.iq_to_bits_batch_dc(captures, p, auto_noise=auto_noise, auto_center=auto_center, center_max_size=center_max_size,
                                       message_length_divisor=message_length_divisor, cap_rows=cap_rows, long_from=long_from)
    elif is_psk(p):
        res = pipe.iq_to_bits_batch_psk(captures, p, auto_noise=auto_noise, auto_center=auto_center, center_max_size=center_max_size,
                                        message_length_divisor=message_length_divisor, cap_rows=cap_rows, long_from=long_from)
    else:
        res = pipe.iq_to_bits_batch_records(captures, p, message_length_divisor, auto_noise=auto_noise, auto_center=auto_center, center_max_size=center_max_size,
                                            cap_rows=cap_rows, long_from=long_from)
    for k in res.truncated:
        res.retry(k)
    return res.messages(sample_rate, timestamps)


def _protocols_each(pipe, captures, params, divisor, sample_rate, timestamps, auto_noise, auto_center, cap_rows, long_from, dc_correction):
    """get_protocols_from_signals_dev with a parameter set per capture"""
    from dataclasses import astuple
    from .batch import check_batch_each_options, is_psk
    from .batch.inputs import _batch_input
    given = _batch_input(pipe, captures)
    n = len(given.caps)
    if len(params) != n:
        raise ValueError(f"params holds one DemodParams per capture ({n}), or is one for all: {len(params)} were given")
    if timestamps is not None and len(timestamps) != n:
        raise ValueError("timestamps holds one entry per capture")
    psk = [k for k in range(n) if is_psk(params[k])]
    rest = [k for k in range(n) if not is_psk(params[k])]
    check_batch_each_options([params[k] for k in rest], len(rest), divisor, auto_center=auto_center)
    out = [None] * n
    stamp = lambda k: 0.0 if timestamps is None else timestamps[k]      # noqa: E731

    def hand_out(res, idx):
        for k in res.truncated:
            res.retry(k)
        for j, k in enumerate(idx):
            out[k] = res.message_data(j, sample_rate, stamp(k))
    if rest:
        sub = captures if len(rest) == n else [given.caps[k] for k in rest]
        if dc_correction:
            sub = pipe.dc_correct_batch(sub)
        hand_out(pipe.iq_to_bits_batch_each(sub, [params[k] for k in rest], auto_noise=auto_noise, message_length_divisor=divisor, cap_rows=cap_rows,
                                            long_from=long_from), rest)
    sets = {}
    for k in psk:
        sets.setdefault(astuple(params[k]), []).append(k)
    for idx in sets.values():
        call = pipe.iq_to_bits_batch_dc if dc_correction else pipe.iq_to_bits_batch_psk
        hand_out(call([given.caps[k] for k in idx], params[idx[0]], auto_noise=auto_noise, message_length_divisor=divisor, cap_rows=cap_rows,
                      long_from=long_from), idx)
    return out


def messages_from_bits(pipe, iq, p, bit_data, pauses, bit_sample_pos, message_length_divisor=1, sample_rate=1e6, timestamp=0.0):
    """The per-message part of get_protocol_from_signal (:256-283) for bits that are already on the host."""
    torch = pipe.torch
    sps = int(p.samples_per_symbol)
    if message_length_divisor > 1 and p.modulation_type == "ASK":
        ensure_message_length_multiple(bit_data, sps, pauses, bit_sample_pos, int(message_length_divisor))
    n = int(iq.shape[0])
    # RSSI: mean of magnitudes_normalized over [middle_bit_pos, middle_bit_pos + samples_per_symbol) -- one gather
    starts = [int(bit_sample_pos[i][int(len(bits) / 2)]) for i, bits in enumerate(bit_data)]
    messages = []
    if starts:
        idx = torch.tensor([s + k for s in starts for k in range(sps) if s + k < n], dtype=torch.int64, device=iq.device)
        got = iq[idx].cpu().numpy()
        lo, hi = _min_max_for_dtype(got.dtype)
        norm = np.sqrt(hi ** 2.0 + lo ** 2.0)
        off = 0
        for i, (bits, pause) in enumerate(zip(bit_data, pauses)):
            cnt = max(0, min(starts[i] + sps, n) - starts[i])
            sl = got[off:off + cnt]
            off += cnt
            if sl.dtype == np.float32:                                   # util.get_magnitudes: fp32 sqrtf, stored as float64
                mags = np.sqrt(sl[:, 0] * sl[:, 0] + sl[:, 1] * sl[:, 1]).astype(np.float64)
            else:                                                        # integer dtypes: C int arithmetic, double sqrt
                a = sl.astype(np.int64)
                s32 = ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
                with np.errstate(invalid="ignore"):
                    mags = np.sqrt(s32.astype(np.float64))
            with np.errstate(invalid="ignore", divide="ignore"):
                rssi = float(np.mean(mags / norm)) if cnt else float("nan")
            messages.append(MessageData(bits, int(pause), bit_sample_pos[i], rssi,
                                        timestamp + bit_sample_pos[i][0] / sample_rate, sps, int(p.bits_per_symbol)))
    return messages
