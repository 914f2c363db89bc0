"""The evaluator's seeding / filter policy without a GPU: tests/golden/G14_eval_policy.json holds, evaluation by evaluation,
what the evaluator decided BEFORE the policy became macr_amd/eval_policy.py (recorder: tests/golden/make_golden_eval_policy.py).
The pure functions must replay every decision and counter of it, and so must the Evaluator that is wired to them."""
import ast
import importlib.util
import json
import os

import pytest
import torch

from macr_amd import eval_policy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_eval_policy", os.path.join(GOLDEN, "make_golden_eval_policy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECORDER = _recorder()
with open(os.path.join(GOLDEN, "G14_eval_policy.json")) as _f:
    TRACE = [RECORDER.unpack(c) for c in json.load(_f)["policy"]]          # (the file holds a list per field)
IDS = ["%s-%d-%s" % (c["filter"], c["n_queries"], "seeds" if c["use_seeds"] else "noseeds") for c in TRACE]


def test_policy_module_imports_neither_torch_nor_the_native_library():
    with open(eval_policy.__file__) as f:
        tree = ast.parse(f.read())
    imported = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {"." * n.level + (n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert imported == {"typing"}, imported


def test_policy_state_is_immutable():
    s = eval_policy.State()
    assert s == (0, 1, 0, 1, 0, 1) and s._fields == ("seed_skip", "seed_backoff", "f16_skip", "f16_backoff", "bf16_skip", "bf16_backoff")
    with pytest.raises(AttributeError):
        s.seed_skip = 3
    assert eval_policy.relist_tolerance(513) == 0 and eval_policy.relist_tolerance(20000) == 1


def test_trace_leaves_the_happy_path():
    """what the recorder asserted when it wrote the file: enough evaluations, every back-off up to 16 and back to 1"""
    assert {c["filter"] for c in TRACE} == {"f16", "bf16", "f32"} and {c["n_queries"] for c in TRACE} == {513, 20000}
    assert {c["use_seeds"] for c in TRACE} == {True, False}
    assert all(len(c["evals"]) >= 200 for c in TRACE)
    for col in (1, 3, 5):
        assert any(16 in v and 1 in v[v.index(16):] for v in ([e[3][col] for e in c["evals"]] for c in TRACE)), col


@pytest.mark.parametrize("cfg", TRACE, ids=IDS)
def test_policy_functions_replay_the_recorded_trace(cfg):
    """eval_policy alone: the evaluator's part -- which path an evaluation takes, whose stats are in flight -- is the few
    lines below"""
    P = eval_policy
    configured, use_seeds, tol = cfg["filter"], cfg["use_seeds"], P.relist_tolerance(cfg["n_queries"])
    s = P.State()
    in_flight = last_seeded = False           # the complete path: a seeded ranking's stats on their way to the host
    host_relisted = 0
    for n, (script, launches, info, counters) in enumerate(cfg["evals"]):
        if script.get("seed_skip0"):
            s = s._replace(seed_skip=0)
        used = P.filter_now(configured, s)
        relisted, fallback = script["relisted"], script["exact_fallback"]
        if script["use_graph"] and script["world"] == 1:            # first-round path
            in_flight = last_seeded = False
            seeded, s = P.seed_first_round(s, use_seeds, script["has_seeds"])
            ran_complete = bool(script.get("graph_off"))
            redone = relisted != 0 and not ran_complete
            if not (redone or ran_complete):
                fallback = 0
            s = P.after_outcome(s, configured, used, seeded, relisted, fallback, redone, tol, ran_complete)
            want_launches = [["first", seeded, used]] + ([["repair", seeded, used]] if redone else [])
            want_info = {"seeded": seeded, "query_blocks_relisted": relisted, "exact_fallback": fallback, "redone": redone,
                         "filter": used}
        else:                                                      # complete path: the filter tiers stay where they are
            previous = None
            if in_flight and P.seeds_allowed(use_seeds, script["world"]):
                in_flight, previous = False, host_relisted if last_seeded else None
            seeded, s = P.seed_complete(s, use_seeds, script["world"], previous, tol)
            seeded = last_seeded = seeded and script["has_seeds"]
            if seeded:
                in_flight, host_relisted = True, relisted
            want_launches = [[None, seeded, used]]
            want_info = {"seeded": seeded, "query_blocks_relisted": relisted, "exact_fallback": fallback, "redone": False}
        assert launches == want_launches, n
        assert info == want_info, n
        assert list(s) == counters, n


def _launch_stub(ev, step, launches):
    """Evaluator._means_launch played from step["script"]: -> (means, graph entry, the complete sequence ran instead)"""
    def stub(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, world, branch=None, repair_of=None, seeded=True,
             mode=None, filter=None):
        s = step["script"]
        launches.append([mode, seeded, filter])
        ran_complete = mode == "first" and bool(s.get("graph_off"))
        if ran_complete:
            ev.use_graph, mode = False, None
            ev._stats_first.zero_()
        if mode == "first":
            ev._stats_first[0], ev._stats_first[1] = s["relisted"], 0
        elif mode == "repair":
            assert repair_of == "first round's buffers"
            ev._stats_first[1] = s["exact_fallback"]
        else:
            ev._stats[0], ev._stats[1] = s["relisted"], s["exact_fallback"]
        entry = (None, None, None, "first round's buffers") if ev.use_graph else None
        return torch.zeros(4, 1, dtype=torch.float64), entry, ran_complete
    return stub


@pytest.mark.parametrize("cfg", TRACE, ids=IDS)
def test_evaluator_replays_the_recorded_trace(cfg):
    """the wiring: the Evaluator itself, its launches replaced by the scripted outcomes, asks for the same launches, reports
    the same last_eval_info() and ends every evaluation with the same six counters"""
    got = RECORDER.drive(cfg, _launch_stub)
    assert len(got) == len(cfg["evals"])
    for n, (g, want) in enumerate(zip(got, cfg["evals"])):
        assert g == want, n


def test_a_copied_evaluator_does_not_share_the_policy_state():
    """tests/test_gpu_product.py clones an evaluator by its __dict__ and evaluates with the clone: the original's counters stay"""
    from macr_amd.evaluator import Evaluator
    ev = Evaluator([[0]], [[0]], 4, "cpu")
    clone = Evaluator.__new__(Evaluator)
    clone.__dict__.update(ev.__dict__)
    clone._seed_skip, clone._f16_backoff = 3, 8
    assert (clone._seed_skip, clone._f16_backoff, clone.filter_now) == (3, 8, ev.filter)
    assert ev._policy == eval_policy.State() and (ev._seed_skip, ev._f16_backoff) == (0, 1)
