"""What the batch entry points refuse, locked word for word (tests/golden/batch_trace/refusals.json; no GPU): every check_batch*_options
function with every option name any of them knows, one unknown name, the parameters it refuses (PSK, or for iq_to_bits_batch_psk not PSK;
for iq_to_bits_batch_dc, which takes both, a modulation no batch demodulates) and a divisor of 0 -- the exception's type and its full
text, or null where the call passes.  tests/test_batch_host.py and its siblings match fragments of these sentences; this file holds them
whole, recorded from the single-module urh_amd/batch.py before its option checks were folded into one loop over the tables.

`PYTHONPATH=.:oracle python tests/test_batch_refusals_host.py` rewrites the fixture from the code as it is."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_trace", "refusals.json")
CHECKS = ("check_batch_options", "check_batch_auto_options", "check_batch_center_options", "check_batch_records_options", "check_batch_psk_options",
          "check_batch_dc_options")
OPTIONS = ("auto_center", "auto_noise", "msg_records", "dc_correction", "no_such_option")
WITH_DIVISOR = ("check_batch_records_options", "check_batch_psk_options", "check_batch_dc_options")


def outcome(call):
    try:
        call()
    except Exception as e:                                       # noqa: BLE001 (whatever it raises is what is recorded)
        return [type(e).__name__, str(e)]
    return None


def all_refusals():
    from urh_amd import batch
    from urh_amd.pipeline import DemodParams
    p = {mod: DemodParams(mod, 1, 0.1, 0.0, 1.0, 5, 100, 0.1, 8, False) for mod in ("FSK", "ASK", "PSK", "QAM")}
    out = {}
    for name in CHECKS:
        check = getattr(batch, name)
        accepted = "PSK" if name == "check_batch_psk_options" else "FSK"
        for mod in p:
            out[f"{name}/modulation/{mod}"] = outcome(lambda: check(p[mod]))
        for option in OPTIONS:
            for value in (True, False):
                out[f"{name}/{option}={value}"] = outcome(lambda: check(p[accepted], **{option: value}))
        if name in WITH_DIVISOR:
            for divisor in (0, 1, 2 ** 30, 2 ** 30 + 1):
                out[f"{name}/message_length_divisor={divisor}"] = outcome(lambda: check(p[accepted], divisor))
    return out


def test_the_refusals_are_the_recorded_ones():
    with open(FIXTURE) as f:
        recorded = json.load(f)
    got = all_refusals()
    assert sorted(got) == sorted(recorded)
    for name in sorted(recorded):
        assert got[name] == recorded[name], name


def test_the_recorded_refusals_hold_the_cases():
    with open(FIXTURE) as f:
        recorded = json.load(f)
    for name in CHECKS:
        assert recorded[f"{name}/no_such_option=True"][0] == "TypeError" and name[len("check_"):-len("_options")] in recorded[f"{name}/no_such_option=True"][1]
        refused = "FSK" if name == "check_batch_psk_options" else "QAM" if name == "check_batch_dc_options" else "PSK"
        assert recorded[f"{name}/modulation/{refused}"][0] == "ValueError", name
        if name in WITH_DIVISOR:
            assert recorded[f"{name}/message_length_divisor=0"][0] == "ValueError" and recorded[f"{name}/message_length_divisor=1"] is None, name
        if name != "check_batch_dc_options":
            assert recorded[f"{name}/dc_correction=True"][0] == "ValueError" and recorded[f"{name}/dc_correction=False"] is None, name
    assert recorded["check_batch_dc_options/modulation/PSK"] is None and recorded["check_batch_dc_options/dc_correction=False"][0] == "TypeError"


if __name__ == "__main__":
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(all_refusals(), indent=0, sort_keys=True) + "\n")
