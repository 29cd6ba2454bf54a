"""The sessions of tests/golden/batch_records/batch_records.npz / .json (tests/golden/make_batch_records_golden.py wrote them with the real
reference, every capture opened alone): loading, the parameters, the reused families of msg_records.npz as ready-made batches, and the
comparison of a batch's messages with a session."""
import json
import os

import numpy as np

import msg_record_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_records")
VARIANTS = {"plain": (False, False), "noise": (True, False), "center": (False, True), "both": (True, True)}      # (auto_noise, auto_center)
KEYS = ("bits", "msg_off", "pauses", "pos", "pos_off", "rssi", "timestamp")
_cache = {}


def _per_capture(i, b, f):
    """the packed arrays of one (session, variant, divisor) as a list per capture of mc.assert_messages' `want` (None: the reference raised)"""
    sizes, at, ints = [int(v) for v in i[:5]], 5, []
    for s in sizes:
        ints.append(i[at:at + s])
        at += s
    n_msg, msg_off, pauses, pos, pos_off = ints
    out, m = [], 0
    for n in n_msg.tolist():
        if n < 0:
            out.append(None)
            continue
        b0, p0 = int(msg_off[m]), int(pos_off[m])
        out.append(dict(bits=b[b0:int(msg_off[m + n])], msg_off=msg_off[m:m + n + 1] - b0, pauses=pauses[m:m + n], pos=pos[p0:int(pos_off[m + n])],
                        pos_off=pos_off[m:m + n + 1] - p0, rssi=f[0, m:m + n], timestamp=f[1, m:m + n]))
        m += n
    return out


def load():
    """{session: dict(meta, iq (the captures back to back), starts, captures [K arrays], names, timestamps [K], want {(variant, divisor):
    [K entries]}, noise / center {variant: float64[K], NaN where not detected})}"""
    if not _cache:
        z = np.load(os.path.join(GOLDEN, "batch_records.npz"))
        meta = json.load(open(os.path.join(GOLDEN, "batch_records.json")))
        for name, m in meta.items():
            iq, starts = z[f"{name}/iq"], z[f"{name}/starts"]
            k = len(starts) - 1
            s = dict(meta=m, iq=iq, starts=starts, captures=[iq[int(a):int(b)] for a, b in zip(starts[:-1], starts[1:])], names=m["captures"],
                     timestamps=[m["timestamp"] + i * m["timestamp_step"] for i in range(k)], want={}, noise={}, center={})
            for v in m["variants"]:
                s["noise"][v], s["center"][v] = z[f"{name}|{v}/nc"]
                for d in m["divisors"]:
                    key = f"{name}|{v}|{d}/"
                    s["want"][(v, int(d))] = _per_capture(z[key + "i"], z[key + "b"], z[key + "f"])
            _cache[name] = s
    return _cache


def names():
    return sorted(load())


def runs():
    """every (session, variant, divisor)"""
    return [(n, v, int(d)) for n in names() for v in load()[n]["meta"]["variants"] for d in load()[n]["meta"]["divisors"]]


def params(meta):
    return mc.params(meta, want_pos=False)


def capture_of(session, name):
    return session["captures"][session["names"].index(name)]


def families():
    """the families of msg_records.npz that share their parameters, as ready-made batches: {name: (cases, meta)}"""
    g = mc.load()
    return {"sa+pad": ([g[f"sa{i}"] for i in range(6)] + [g["pad"]], g["sa0"]["meta"]), "sf": ([g[f"sf{i}"] for i in range(4)], g["sf0"]["meta"])}


def assert_session(got, session, variant, divisor, what):
    """got: BatchBits.messages()'s list of MessageData lists against the session's record, capture by capture"""
    want = session["want"][(variant, divisor)]
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        mc.assert_messages(g, w, (what, session["names"][k]))
