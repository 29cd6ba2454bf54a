"""What each batch entry point refuses, in sentences that say what to call instead: the tables, one walk over a table, one divisor check."""
from collections import namedtuple
from dataclasses import replace

from .. import _lib
from ..signal_functions import mod_code

# the refusals of dc_correction name the entry point that does it, then say what they always said
_DC_FIRST = "call iq_to_bits_batch_dc(captures, p, ...), which removes every capture's means on the device in two more launches; apart from that method "

_NOT_IN_A_BATCH = {
    "auto_center": "iq_to_bits_batch slices every capture with p.center: call iq_to_bits_batch_center(captures, p, auto_noise=False), which detects a center "
                   "per capture (or call iq_to_bits(..., auto_center=True) per capture, or a CaptureStream(auto_center=True))",
    "auto_noise": "iq_to_bits_batch gates every capture with p.noise_threshold: call iq_to_bits_batch_auto(captures, p), which detects a threshold per capture",
    "msg_records": "iq_to_bits_batch computes no message records: call iq_to_bits_batch_records(captures, p), which queues them behind the batch (or call "
                   "iq_to_bits(..., msg_records=True) per capture, or a CaptureStream(msg_records=True))",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., dc_correction=True) per capture, or a CaptureStream(dc_correction=True)",
}

_NOT_IN_A_BATCH_AUTO = {
    "auto_center": "iq_to_bits_batch_auto slices every capture with p.center: call iq_to_bits_batch_center(captures, p), which detects a threshold and a "
                   "center per capture (or call iq_to_bits(..., auto_noise=True, auto_center=True) per capture, or a CaptureStream)",
    "msg_records": "iq_to_bits_batch_auto computes no message records: call iq_to_bits_batch_records(captures, p, auto_noise=True), which queues them behind "
                   "the batch (or call iq_to_bits(..., auto_noise=True, msg_records=True) per capture, or a CaptureStream)",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., auto_noise=True, dc_correction=True) per capture, or a CaptureStream",
}

_NOT_IN_A_BATCH_CENTER = {
    "msg_records": "iq_to_bits_batch_center computes no message records: call iq_to_bits_batch_records(captures, p, auto_noise=..., auto_center=True), which "
                   "queues them behind the batch (or call iq_to_bits(..., auto_center=True, msg_records=True) per capture, or a CaptureStream)",
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., auto_center=True, dc_correction=True) per capture, or a CaptureStream",
}

_NOT_IN_A_BATCH_RECORDS = {
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., msg_records=True, dc_correction=True) per capture, or a CaptureStream",
}

_NOT_IN_A_BATCH_PSK = {
    "dc_correction": _DC_FIRST + "a batch does not remove the captures' means: call iq_to_bits(..., dc_correction=True) per capture, or a CaptureStream(dc_correction=True)",
}


_NOT_IN_A_BATCH_EACH = {
    "auto_center": "iq_to_bits_batch_each slices every capture with the center of its own params[k] (estimated parameters already carry a center): to "
                   "detect a center per capture call iq_to_bits_batch_center(captures, p), which takes one parameter set for all",
    "dc_correction": "iq_to_bits_batch_each does not remove the captures' means: call dc_correct_batch(captures) first and hand what it returns, "
                     "(iq_cat, starts), to iq_to_bits_batch_each as the captures -- two more launches, whatever the number of captures",
}


# the options of a batch as its entry point settled them, after its checks -- what _batch runs and what retry(k) runs again: center -- a center
# per capture, detected with max_size, cap_tie the counts its tie pool holds (None: the default); records -- the message_length_divisor, or None
BatchOptions = namedtuple("BatchOptions", "auto_noise center max_size cap_tie records psk dc", defaults=(False, False, None, None, None, False, False))


def _refuse(entry, table, options):
    """an option the entry point does not know is a TypeError; one of its table that is set, a ValueError with the table's sentence"""
    for name, value in options.items():
        if name not in table:
            raise TypeError(f"{entry}() got an unexpected keyword argument '{name}'")
        if value:
            raise ValueError(f"{name} is not an option of a batch: {table[name]}")


def _check_divisor(message_length_divisor):
    if not 1 <= int(message_length_divisor) <= 1 << 30:
        raise ValueError("message_length_divisor must be at least 1 (and at most 2 ** 30)")


def is_psk(p) -> bool:
    return mod_code(p.modulation_type)[0] == _lib.MOD_PSK


def as_fsk(p):
    """PSK parameters recoded as FSK for what reads no modulation but through the noise value, which the two share (-4): the plan (lengths,
    tolerance, samples per symbol, bits per symbol), the qad-input walk (no ASK rule) and the records (no ASK padding)"""
    return replace(p, modulation_type="FSK") if is_psk(p) else p


def check_batch_options(p, **options):
    """what a batch does not do raises ValueError with a sentence that says what to call instead (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch", _NOT_IN_A_BATCH, options)
    mod, _ = mod_code(p.modulation_type)
    if mod not in (_lib.MOD_ASK, _lib.MOD_FSK):
        raise ValueError(f"this batch demodulates ASK and FSK, not {p.modulation_type}: for PSK call iq_to_bits_batch_psk(captures, p), which runs a "
                         "Costas loop per capture in one launch (or call iq_to_bits per capture, or push the captures through a CaptureStream)")


def check_batch_auto_options(p, **options):
    """what iq_to_bits_batch_auto does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_auto", _NOT_IN_A_BATCH_AUTO, options)
    check_batch_options(p)


def check_batch_center_options(p, **options):
    """what iq_to_bits_batch_center does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_center", _NOT_IN_A_BATCH_CENTER, options)
    check_batch_options(p)


def check_batch_records_options(p, message_length_divisor=1, **options):
    """what iq_to_bits_batch_records does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_records", _NOT_IN_A_BATCH_RECORDS, options)
    check_batch_options(p)
    _check_divisor(message_length_divisor)


def check_batch_psk_options(p, message_length_divisor=None, **options):
    """what iq_to_bits_batch_psk does not do raises ValueError with a sentence (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_psk", _NOT_IN_A_BATCH_PSK, options)
    if not is_psk(p):
        raise ValueError(f"iq_to_bits_batch_psk demodulates PSK, not {p.modulation_type}: for ASK and FSK call iq_to_bits_batch or one of its siblings "
                         "(iq_to_bits_batch_auto, iq_to_bits_batch_center, iq_to_bits_batch_records)")
    if message_length_divisor is not None:
        _check_divisor(message_length_divisor)


def check_batch_dc_options(p, message_length_divisor=None, **options):
    """iq_to_bits_batch_dc takes the options of its signature alone: anything else is a TypeError, a divisor below 1 and a modulation no batch
    demodulates a ValueError (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_dc", {}, options)
    if is_psk(p):
        check_batch_psk_options(p)
    else:
        check_batch_options(p)
    if message_length_divisor is not None:
        _check_divisor(message_length_divisor)


def check_batch_each_options(params, k, message_length_divisor=None, **options):
    """what iq_to_bits_batch_each does not do raises ValueError with a sentence that says what to call instead; returns the K DemodParams, a
    single one broadcast (host arithmetic: no GPU needed)"""
    _refuse("iq_to_bits_batch_each", _NOT_IN_A_BATCH_EACH, options)
    if hasattr(params, "modulation_type"):
        params = [params] * int(k)
    params = list(params)
    if len(params) != int(k):
        raise ValueError(f"params holds one DemodParams per capture ({int(k)}), or is one for all: {len(params)} were given")
    for i, p in enumerate(params):
        mod, _ = mod_code(p.modulation_type)
        if mod not in (_lib.MOD_ASK, _lib.MOD_FSK):
            raise ValueError(f"iq_to_bits_batch_each demodulates ASK and FSK, not {p.modulation_type} (params[{i}]): split the PSK captures off and call "
                             "iq_to_bits_batch_psk(captures, p) per PSK parameter set, which runs a Costas loop per capture in one launch")
    if message_length_divisor is not None:
        _check_divisor(message_length_divisor)
    return params
