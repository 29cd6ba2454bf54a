"""The order in which ShardedPipeline calls its engine and its communicator, locked against recorded traces
(tests/golden/shard_trace/traces.json), and the public surface of urh_amd.sharding.  The traces were recorded with this file's recorder
against the single-module urh_amd/sharding.py that the package replaced: a rank that entered one collective more or fewer than the others,
or in another place, would hang a node, and no bit-exact comparison of results shows a call that moved.  No GPU: the model engines of the
host suite over ThreadComm, world size 3.

`PYTHONPATH=.:oracle python tests/test_shard_call_trace.py` rewrites the fixture from the code as it is -- only from a commit whose call order is known good."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dc_cases
import model_shard_auto as A
import model_shard_dc as MD
import model_shard_estimators as M
import model_shard_msg_records as MR
import msg_record_cases as mc
from urh_amd import sharding as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_trace", "traces.json")
WORLD = 3
N = 6_000
RECORD_EDGES = {"window": [0, 300, 532, 806], "no_window": [0, 250, 490, 806]}        # fixture "pad": a first window across ranks 1 | 2; none


class Recorder:
    """forwards to `inner` and notes the name of every method called; what `inner` lacks stays missing (the orchestration's hasattr)"""

    def __init__(self, inner, log, prefix, only=None):
        self.__dict__.update(_inner=inner, _log=log, _prefix=prefix, _only=only)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr) or (self._only is not None and name not in self._only):
            return attr

        def call(*args, **kw):
            self._log.append(self._prefix + name)
            return attr(*args, **kw)
        return call


def traced(world, engine_for, work, timeout=60):
    """work(rank, pipeline) on `world` ranks -> (per rank: the ordered names of the calls, then "raises <type>" where it raised; results)"""
    logs = [[] for _ in range(world)]

    def body(r, comm):
        sp = S.ShardedPipeline(Recorder(engine_for(r), logs[r], "engine."), Recorder(comm, logs[r], "comm.", ("all_gather", "all_gather_start")))
        return work(r, sp)
    out, err = M.run_ranks(world, body, timeout)
    for r, e in enumerate(err):
        if e is not None:
            logs[r].append("raises " + type(e).__name__)
    return logs, out


class HookedAutoEngine(A.ModelAutoEngine):
    """the model with the optional hooks of the GPU engine: every hasattr branch of the fused pass is taken"""

    def halo_context(self):
        return contextlib.nullcontext()

    def tail_context(self):
        return contextlib.nullcontext()

    def halo_view(self, left_halo):
        return left_halo

    def runs_begin(self, *args):
        pass

    def runs_launch(self, *args):
        pass


class StubPskEngine(M.ModelEstimatorEngine):
    """a PSK engine without arithmetic: a hand-built Costas summary (test_costas_compose.chain), the end state it hands over, and a
    two-level demodulated signal for detect_center"""

    def __init__(self, summary, end, qad):
        self.summary, self.end_bits, self.qad = summary, end, qad
        self.end = torch.zeros(2, dtype=torch.int32)

    def costas_spec(self, iq_local, left_raw, pos_base, n_total, rank, world, p):
        return torch.from_numpy(self.summary.copy())

    def costas_resolve(self, start):
        self.end.copy_(torch.from_numpy(np.array(self.end_bits, np.uint32).view(np.int32)))

    def costas_end(self):
        return self.end

    def costas_stats(self):
        return 0, 0, 0, 0

    def costas_last(self):
        return torch.from_numpy(self.qad[-1:].copy())

    def costas_qad(self):
        return self.qad

    def set_center(self, center):
        pass

    def runs(self, *args):
        return torch.zeros(9, dtype=torch.int64)

    def rows(self, summaries):
        return None

    def bits_prepare(self, merged_all):
        return torch.zeros(3, dtype=torch.int64)

    def bits_finish(self, flags_all):
        return {}


def equal_cuts(n, world):
    per = -(-n // world)
    return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(world)]


def pass_cases(oracle):
    """the fused pass and iq_to_bits_auto on the model of the engine"""
    bounds = S.shard_bounds(N, WORLD)
    out = {}
    for mod in ("ASK", "FSK"):
        iq, p = A.message_capture(N, mod, seed=3), A.params(mod)

        def halo(r):
            return iq[bounds[r][0] - 2:bounds[r][0]] if r else None

        def fused(kind, halo_given):
            def work(r, sp):
                a, b = bounds[r]
                kw = dict(halo_given=True, left_halo=halo(r)) if halo_given else {}
                sp.iq_to_bits(iq[a:b], p, pos_base=a, n_total=N, **kw)
            return traced(WORLD, lambda r: kind(oracle.afp_demod), work)[0]
        out[f"{mod}/halo_exchange"] = fused(A.ModelAutoEngine, False)
        out[f"{mod}/halo_given"] = fused(A.ModelAutoEngine, True)
        out[f"{mod}/halo_exchange/hooks"] = fused(HookedAutoEngine, False)
        out[f"{mod}/halo_given/hooks"] = fused(HookedAutoEngine, True)
        for auto_noise in (False, True):
            for auto_center in (False, True):
                for halo_given in (False, True):
                    def work(r, sp):
                        a, b = bounds[r]
                        sp.iq_to_bits_auto(iq[a:b], p, auto_noise=auto_noise, auto_center=auto_center, pos_base=a, n_total=N, halo_given=halo_given,
                                           left_halo=halo(r) if halo_given else None)
                        return sp.last_auto["all_gathers"]
                    logs, counts = traced(WORLD, lambda r: A.ModelAutoEngine(oracle.afp_demod), work)
                    assert counts == [sum(c.startswith("comm.") for c in log) for log in logs]          # last_auto counts what was entered
                    out[f"{mod}/auto/noise={int(auto_noise)}/center={int(auto_center)}/halo_given={int(halo_given)}"] = logs
    return out


def dc_cases_traces():
    out = {}
    offset = (0.5 + 0.1 * np.random.default_rng(1).standard_normal((30_000, 2))).astype(np.float32)
    inputs = {"int16": (dc_cases.generic(np.int16, N + 1), equal_cuts(N + 1, WORLD)),
              "float32_hand_over": (dc_cases.F32_CASES["zero_mean_spiked"](30_000), equal_cuts(30_000, WORLD)),      # every later rank hands over
              "float32_records_hold": (offset, [(0, 20_000), (20_000, 25_000), (25_000, 30_000)])}       # short later shards: the guesses hold
    for name, (x, cuts) in inputs.items():

        def work(r, sp):
            a, b = cuts[r]
            sp.dc_correct(x[a:b].copy(), pos_base=a, n_total=len(x), also=(x[:2].copy(),) if r == 1 else ())
            return sp.last_dc["all_gathers"]
        logs, counts = traced(WORLD, lambda r: MD.ModelDcEngine(), work)
        assert counts == [sum(c.startswith("comm.") for c in log) for log in logs]
        out[f"dc/{name}"] = logs
    return out


def records_cases(oracle):
    g = mc.load()["pad"]
    m = g["meta"]
    qad = oracle.afp_demod(g["iq"], m["noise_threshold"], m["modulation_type"], 2 ** m["bits_per_symbol"], m["costas_loop_bandwidth"])
    p, n = mc.params(m), len(g["iq"])
    out = {}
    for name, edges in RECORD_EDGES.items():
        assert edges[-1] == n

        def work(r, sp):
            a, b = edges[r], edges[r + 1]
            piece = sp.iq_to_bits(qad[a:b], p, pos_base=a, n_total=n)
            sp.message_records(g["iq"][a:b], piece, p, 8, pos_base=a, n_total=n)
            return sp.last_records
        logs, last = traced(WORLD, lambda r: MR.pass_and_records_engine(tile=32, span=8, chunk_tiles=2), work)
        assert all(x == last[0] for x in last) and last[0]["all_gathers"] == (3 if name == "window" else 2), (name, last)
        assert (last[0]["windows"] > 0) == (name == "window"), (name, last)
        out[f"records/{name}"] = logs
    return out


def psk_cases():
    from test_costas_compose import chain
    from urh_amd.pipeline import DemodParams
    p = DemodParams("PSK", 2, 0.1, 0.0, 1.5, 5, 100, 0.1, 8, True)
    bounds = S.shard_bounds(N, WORLD)
    summ, states = chain(WORLD, seed=3)
    out = {}
    for name, broken in (("chain_holds", []), ("hand_over_at_rank_1", [1]), ("hand_over_at_ranks_0_and_1", [0, 1])):
        sm = summ.copy()
        for r in broken:
            w = sm[r].view(np.uint32).copy()
            w[32] = 0xFFFFFFFF
            sm[r] = w.view(np.uint8)
        for auto_center in (False, True):
            def work(r, sp):
                a, b = bounds[r]
                left_raw = torch.zeros((S.costas_halo_samples(p.costas_loop_bandwidth, a), 2)) if r else None
                if auto_center:
                    sp.iq_to_bits_auto(torch.zeros((b - a, 2)), p, auto_center=True, pos_base=a, n_total=N, left_raw=left_raw)
                else:
                    sp.iq_to_bits(torch.zeros((b - a, 2)), p, pos_base=a, n_total=N, left_raw=left_raw)
                return sp.last_costas["rounds"]
            logs, rounds = traced(WORLD, lambda r: StubPskEngine(sm[r], states[r + 1], M.two_level(2_000, 7 + r)), work)
            assert rounds == [1 + len(broken)] * WORLD
            out[f"PSK/{name}/auto_center={int(auto_center)}"] = logs

    # the stand-in of tests/test_costas_compose.py: a rank without its left_raw raises before it touches the engine or the communicator
    class NoComm:
        rank, world = 1, 2

        def all_gather(self, t):
            raise AssertionError("a collective was entered")
        all_gather_start = all_gather

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was used: {name}")
    log = []
    sp = S.ShardedPipeline(Recorder(NoEngine(), log, "engine."), Recorder(NoComm(), log, "comm.", ("all_gather", "all_gather_start")))
    with pytest.raises(ValueError, match="2999"):
        sp.iq_to_bits(torch.zeros((3_000, 2)), p, pos_base=3_000, n_total=N, left_raw=torch.zeros((100, 2)))
    out["PSK/refusal"] = [log + ["raises ValueError"]]
    return out


def all_traces(oracle):
    out = {}
    out.update(pass_cases(oracle))
    out.update(dc_cases_traces())
    out.update(records_cases(oracle))
    out.update(psk_cases())
    return out


@pytest.fixture(scope="module")
def traces(oracle):
    return all_traces(oracle)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_cases_are_the_recorded_ones(traces, recorded):
    assert sorted(traces) == sorted(recorded)


def test_call_order_equals_the_recorded_traces(traces, recorded):
    for name in sorted(recorded):
        assert traces[name] == recorded[name], name


def test_the_recorded_traces_hold_the_cases(recorded):
    """the grounds the cases were chosen for are in the fixture itself"""
    def gathers(name):
        return [sum(c.startswith("comm.") for c in log) for log in recorded[name]]
    assert gathers("dc/int16") == [1] * WORLD and gathers("dc/float32_records_hold") == [2] * WORLD
    assert gathers("dc/float32_hand_over")[0] > 2 and len(set(gathers("dc/float32_hand_over"))) == 1          # at least one hand-over round
    assert gathers("PSK/hand_over_at_rank_1/auto_center=0")[0] == gathers("PSK/chain_holds/auto_center=0")[0] + 1
    assert gathers("ASK/halo_exchange") == [4] * WORLD and gathers("FSK/halo_exchange") == [3] * WORLD         # ASK: the merge gather
    assert gathers("FSK/halo_given") == [2] * WORLD
    assert "comm.all_gather_start" in recorded["FSK/halo_exchange"][0] and "engine.runs_begin" in recorded["FSK/halo_exchange/hooks"][0]
    assert "engine.runs_launch" in recorded["FSK/halo_given/hooks"][1] and "engine.halo_view" in recorded["FSK/halo_given/hooks"][1]
    assert gathers("records/window") == [4 + 3] * WORLD and gathers("records/no_window") == [4 + 2] * WORLD    # the ASK pass's four, then the records'
    assert recorded["PSK/refusal"] == [["raises ValueError"]]
    for name, logs in recorded.items():
        assert all([c for c in log if c.startswith("comm.")] == [c for c in logs[0] if c.startswith("comm.")] for log in logs), name


# ---- the surface: every public module-level name of the single module the package replaced ------------------------------------------------
SURFACE = """COSTAS_START COSTAS_SUMMARY_BYTES DC_IDENTITY HIST_GATHER_BINS PW_LEAF PW_PIECE PW_REC_FIRST PW_REC_HEAD PW_REC_LAST PW_REC_PIECES
PW_REC_TAIL REC_FIRST_PAUSE REC_FIRST_WORDS REC_HEAD_BITS REC_HEAD_POS REC_HELD REC_N_LOCAL REC_N_MSG REC_N_POS REC_POS_BASE REC_SUMMARY_WORDS
REC_TAIL_BITS REC_TAIL_POS RcclComm ShardedPipeline ThreadComm TorchDistComm center_parts costas_compose costas_exchange costas_halo_samples
dc_compose message_data minmax_combine pack_costas_summary pairwise_combine pairwise_inside_pieces pairwise_leaf_sum pairwise_piece_leaves
pairwise_record_words pairwise_tree records_plan records_requests records_windows shard_bounds stitch stitch_records""".split()


def test_every_public_name_is_importable():
    for name in SURFACE:
        assert hasattr(S, name), name
    assert S.RcclComm.INIT_TIMEOUT_S == 120.0 and S.RcclComm.last_fallback_reason is None
    assert S.COSTAS_START == (0x00000000, 0x3FC00000) and S.REC_N_POS == 9 and S.HIST_GATHER_BINS == 1 << 22


def test_import_needs_no_torch_distributed():
    """in a process where torch.distributed cannot be imported at all"""
    code = ("import sys; sys.modules['torch.distributed'] = None; import urh_amd.sharding as S; "
            "assert S.ShardedPipeline and S.RcclComm and S.stitch; print('imported')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "imported" in res.stdout, res.stderr


if __name__ == "__main__":
    import urh_oracle
    urh_oracle.lib()
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    text = json.dumps(all_traces(urh_oracle), indent=0, sort_keys=True)
    with open(FIXTURE, "w") as f:
        f.write(text + "\n")
