#!/usr/bin/env python3
"""Run the REAL reference (where it is built) on the captures of tests/estimate_route_cases.py -> tests/golden/estimate_routes.json.

Per capture of every scenario: AutoInterpretation.estimate(capture, noise, modulation) with the scenario's arguments (the dict, or null), and
what the reference's own pieces say about the capture's messages, so that a test can tell from the record which route a capture must take:
  segments        messages segment_messages_from_magnitudes finds (before the OOK merge)
  modulation      the modulation the per-message loop runs with: given, or detected
  messages        messages the per-message loop walks (after the OOK merge), and "ranges": the first and last of them
  bins_over_pool  messages whose detect_center histogram has more than 4096 bins
  tied            messages with at least three peaks in that histogram whose second and third are equally populated
  outlasting      messages without a plateau boundary in [25 % of the message, 25 % + 65 536) although the message goes on beyond that
  equal_counts    messages in whose divisor histogram the walk of get_bit_length_from_plateau_lengths meets two equal counts
  plateaus        plateau lengths get_plateau_lengths returns, over all messages
Only results go into the file, never a capture.  The recorder refuses to write when a scenario's answer is None where a dict is due, when the
reference detects PSK for a capture of a session without a modulation (its PSK estimate reads uninitialised memory), or when a scenario does
not meet the condition of a route it is listed for.

    python tests/golden/make_estimate_routes_golden.py            record
    python tests/golden/make_estimate_routes_golden.py --search   print seeds of estimate_route_cases.noisy_capture that tie
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_python  # noqa: E402

ref_python.setup()
from urh.ainterpretation import AutoInterpretation as AI  # noqa: E402
from urh.cythonext import auto_interpretation as c_auto_interpretation  # noqa: E402
from urh.cythonext import signal_functions  # noqa: E402
from urh.signalprocessing.IQArray import IQArray  # noqa: E402

import estimate_route_cases as rc  # noqa: E402

POOL_BINS, WINDOW = 4096, 1 << 16


def _histogram(rect):
    """detect_center's histogram (AutoInterpretation.py:226-248): (counts, number of bins) -- counts None without one or beyond the pool"""
    rect = rect[rect > -4]
    rect = rect[int(0.05 * len(rect)):int(0.95 * len(rect))]
    if len(rect) == 0:
        return None, 0
    step = float(np.var(rect))
    try:
        with np.errstate(all="ignore"):
            edges = np.arange(float(rect.min()), float(rect.max()) + step, step)
        if len(edges) - 1 > POOL_BINS:
            return None, len(edges) - 1
        y, _ = np.histogram(rect, bins=edges)
    except (ZeroDivisionError, ValueError):
        return None, 0
    return y, len(y)


def _second_and_third_peak_tie(y):
    w = max(2, int(0.05 * len(y)) + 1) - 1
    p = np.concatenate([np.zeros(w, y.dtype), y, np.zeros(w, y.dtype)])
    win = np.lib.stride_tricks.sliding_window_view(p, 2 * w + 1)
    others = np.delete(win, w, axis=1).max(axis=1)
    peaks = np.sort(y[(y > 0) & (y > others)])[::-1]
    return len(peaks) >= 3 and peaks[1] == peaks[2]


def _equal_counts(merged):
    merged = np.array(merged, dtype=np.uint64)
    AI.round_plateau_lengths(merged)
    hist = np.asarray(c_auto_interpretation.get_threshold_divisor_histogram(merged))
    counts = np.sort(hist[hist > 0])[::-1]
    if len(counts) == 0:
        return True
    for i in range(1, len(counts)):
        if counts[i] < 0.25 * counts[0]:
            break
        if counts[i] == counts[i - 1]:
            return True
    return False


def anatomy(iq, noise, modulation):
    """the counts above for one capture with the noise threshold and the modulation the estimate ends up with"""
    out = dict(segments=0, messages=0, ranges=[], bins_over_pool=0, tied=0, outlasting=0, equal_counts=0, plateaus=0)
    if len(iq) == 0 or modulation is None:
        return out
    arr = IQArray(np.array(iq))
    msgs = AI.segment_messages_from_magnitudes(arr.magnitudes, noise_threshold=noise)
    out["segments"] = len(msgs)
    if modulation == "OOK":
        msgs = AI.merge_message_segments_for_ook(msgs)
    out["messages"] = len(msgs)
    out["ranges"] = [[int(a), int(b)] for a, b in (msgs[:1] + msgs[-1:] if len(msgs) > 1 else msgs)]
    data = signal_functions.afp_demod(arr.data, noise, "ASK" if modulation in ("OOK", "ASK") else modulation, 2)
    for start, end in msgs:
        rect = data[start:end]
        y, bins = _histogram(rect)
        out["bins_over_pool"] += bins > POOL_BINS
        if y is not None and _second_and_third_peak_tie(y):
            out["tied"] += 1
        center = AI.detect_center(rect)
        if center is None:
            continue
        n, limit = len(rect), (25 * len(rect)) // 100
        if n > limit + WINDOW:
            below = rect[:limit + WINDOW] <= np.float32(center)
            edges = np.nonzero(below[1:] != below[:-1])[0] + 1
            out["outlasting"] += not (edges >= limit).any()
        plateaus = c_auto_interpretation.get_plateau_lengths(rect, center, percentage=25)
        out["plateaus"] += len(plateaus)
        tolerance = AI.estimate_tolerance_from_plateau_lengths(plateaus)
        merged = AI.merge_plateau_lengths(plateaus, tolerance=tolerance or 0)
        if len(merged) >= 2 and _equal_counts(merged):
            out["equal_counts"] += 1
    return {k: (int(v) if not isinstance(v, list) else v) for k, v in out.items()}


def plain(r):
    return None if r is None else {key: (float(v) if key in ("center", "noise") else (int(v) if key != "modulation_type" else v)) for key, v in r.items()}


def search():
    for mod in ("FSK", "ASK"):
        found = {"tied": [], "equal_counts": []}
        for seed in range(8400, 8500):
            iq = rc.noisy_capture(mod, seed)
            r = AI.estimate(np.array(iq), modulation=mod)
            if r is None:
                continue
            a = anatomy(iq, r["noise"], mod)
            for key in found:
                if a[key] and not a["bins_over_pool"]:
                    found[key].append((seed, a["tied"], a["equal_counts"]))
        print(mod, {k: v[:6] for k, v in found.items()})


def record():
    out = {}
    for sname, s in rc.scenarios().items():
        k = len(s["captures"])
        noise, mods = rc.per_capture(s["noise"], k), rc.per_capture(s["modulation"], k)
        res = []
        for i, (iq, nz, m) in enumerate(zip(s["captures"], noise, mods)):
            iq = np.array(iq)
            seen = m
            if len(iq):
                arr = IQArray(iq)
                thr = AI.detect_noise_level(arr.magnitudes) if nz is None else nz
                if m is None:
                    seen = AI.detect_modulation_for_messages(arr, AI.segment_messages_from_magnitudes(arr.magnitudes, noise_threshold=thr))
                    assert seen != "PSK", f"{sname}[{i}]: the reference detects PSK: choose another seed"
            else:
                thr = nz
            r = plain(AI.estimate(iq, noise=nz, modulation=m)) if len(iq) else None
            entry = dict(estimate=r, modulation=seen, **anatomy(iq, thr, seen))
            assert r is not None or (sname.startswith("session-pooled") and entry["messages"] == 0), f"{sname}[{i}]: the reference gives None"
            res.append(entry)
        out[sname] = res
        total = {key: sum(c[key] for c in res) for key in ("segments", "messages", "bins_over_pool", "tied", "outlasting", "equal_counts", "plateaus")}
        print(sname, total, [c["estimate"] for c in res][:3])
        for route, ok in (("R1", total["segments"] > 4096), ("R4", total["messages"] > 4096), ("R5", total["bins_over_pool"] > 0),
                          ("R6", total["tied"] > 0), ("R7", total["outlasting"] > 0), ("R8", total["equal_counts"] > 0),
                          ("R2", total["messages"] > rc.OOK_MERGED_CAP), ("R9", sum(c["messages"] for c in res if c["modulation"] == "FSK") > 4096)):
            assert route not in s["routes"] or ok, f"{sname} does not meet the condition of {route}: {total}"
    with open(rc.RECORD, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(name) + ": [\n" + ",\n".join(" " + json.dumps(c, sort_keys=True) for c in out[name]) + "\n]"
                                    for name in sorted(out)) + "\n}\n")             # (a capture per line)
    print(os.path.getsize(rc.RECORD), "bytes")


if __name__ == "__main__":
    search() if "--search" in sys.argv else record()
