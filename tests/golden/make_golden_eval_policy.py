"""Recorder of tests/golden/G14_eval_policy.json: what the evaluator's seeding / filter policy decides, evaluation by
evaluation, and which kernels an evaluation launches.

RUN AT THE PARENT COMMIT of the change that split macr_amd/evaluator.py into the policy module (eval_policy.py), the
launch arguments and the graph cache: the file pins what the evaluator did BEFORE that refactor, and
tests/test_eval_policy_cpu.py / tests/test_gpu_product.py hold the refactored code to it.  `launch_stub_parent` below
speaks the parent's interface (results left on the evaluator); the tests pass `drive` a stub for today's.

    python tests/golden/make_golden_eval_policy.py          # key "policy": no GPU needed
    python tests/golden/make_golden_eval_policy.py --gpu    # key "kernel_names": one MI355X

Each part rewrites its own key of the JSON and leaves the other alone.

"policy": a list of configurations {"filter", "n_queries", "use_seeds", ...}.  The evaluator is built on the CPU, told
that it lives on a GPU, and its launches are replaced by a stub that plays a scripted outcome, so the host code between
the launches -- all of the policy -- runs as it does in production.  In memory an evaluation is
    [script, launches, info, counters]
script   = {"relisted": query blocks the first round (or the complete ranking) lists twice, "exact_fallback": of the repair
            round (or the complete ranking), "has_seeds", "use_graph", "world", and, where present, "graph_off": graph
            replay is switched off during this first round, "seed_skip0": `ev._seed_skip = 0` before it (bench.py does)}
launches = [[mode, seeded, filter], ...] as requested of _means_launch
info     = last_eval_info()
counters = [_seed_skip, _seed_backoff, _f16_skip, _f16_backoff, _bf16_skip, _bf16_backoff] after the evaluation
and the file holds one list per field instead of one record per evaluation (pack / unpack below; "graph_off" and
"seed_skip0" as the evaluations' numbers; "modes" "f" / "fr" / "c" = first round, first and repair round, complete).
"""
import json
import os
import random
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "G14_eval_policy.json")
COUNTERS = ("_seed_skip", "_seed_backoff", "_f16_skip", "_f16_backoff", "_bf16_skip", "_bf16_backoff")
CONFIGS = [("f16", 513, True), ("bf16", 20000, True), ("f32", 513, True), ("f16", 20000, False)]
INFO = ("seeded", "query_blocks_relisted", "exact_fallback", "redone", "filter")
SCRIPT = ("relisted", "exact_fallback", "has_seeds", "use_graph", "world")
MODES = {"f": ["first"], "fr": ["first", "repair"], "c": [None]}


# ----------------------------------------------------------------------------- the script
def make_script(seed):
    """~280 evaluations: good and bad stretches long enough for every back-off to climb to 16 and to come back."""
    rs = random.Random(seed)
    ev = []

    def add(n, bad, fallback_p, relisted=(2, 5), **kw):
        for _ in range(n):
            is_bad = rs.random() < bad
            e = {"relisted": rs.randint(*relisted) if is_bad else 0,
                 "exact_fallback": int(is_bad and rs.random() < fallback_p), "has_seeds": True, "use_graph": True, "world": 1}
            e.update(kw)
            ev.append(e)

    add(20, 0.0, 0.0)                              # first-round path, a model that drifts: seeds hold
    ev[0]["has_seeds"] = False                     # (nothing to seed the first ranking with)
    add(70, 1.0, 0.85)                             # a model that jumps every time, scores packed too close for f16 and bf16
    ev[45]["seed_skip0"] = True                    # the benchmark's write, in the middle of a back-off
    for k in (30, 31, 32, 60, 61):                 # (no seeds for this K and shard while a back-off runs: it runs on)
        ev[k]["has_seeds"] = False
    add(50, 0.0, 0.0)                              # ... settles: every back-off returns to 1
    ev[100]["has_seeds"] = False                   # (set_local_items dropped the seeds)
    add(30, 1.0, 0.0, relisted=(1, 1))             # one block listed twice, no fallback: within the tolerance of 20000 queries
    ev[150]["seed_skip0"] = True
    add(20, 0.5, 0.5)
    add(1, 1.0, 1.0, graph_off=True)               # graph replay switched off during a first round
    add(25, 1.0, 0.5, use_graph=False)             # the complete path, one rank: stale seeds ...
    add(15, 0.0, 0.0, use_graph=False)             # ... and good ones
    ev[-5]["seed_skip0"] = True
    add(20, 0.5, 0.5, use_graph=False, world=2)    # two ranks: never seeded
    add(5, 1.0, 0.0, use_graph=False)              # (leaves a stats copy in flight for the first-round path to drop)
    add(25, 0.3, 0.3)                              # the first-round path again
    return ev


# ----------------------------------------------------------------------------- the driver
class _Event(object):
    def record(self): pass
    def synchronize(self): pass


class _Stream(object):
    cuda_stream = 0
    def synchronize(self): pass


def launch_stub_parent(ev, step, launches):
    """Evaluator._means_launch of the parent commit, played from step["script"]"""
    def stub(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, world, seeded, mode=None, branch=None):
        s = step["script"]
        launches.append([mode, bool(seeded), ev.filter_now])
        ev._last_entry = None
        if mode == "first" and s.get("graph_off"):
            ev.use_graph = False
            ev._topk_mode = None
            ev._stats_first.zero_()
            ev._complete_ran = True
            mode = None
        elif ev.use_graph:
            ev._last_entry = (None, None, None, ())
        if mode == "first":
            ev._stats_first[0], ev._stats_first[1] = s["relisted"], 0
        elif mode == "repair":
            ev._stats_first[1] = s["exact_fallback"]
        else:
            ev._stats[0], ev._stats[1] = s["relisted"], s["exact_fallback"]
        return torch.zeros(4, 1, dtype=torch.float64)
    return stub


def drive(cfg, launch_stub=launch_stub_parent):
    """Runs cfg["evals"][i][0] (the scripts) through an Evaluator; -> [[script, launches, info, counters], ...]"""
    from macr_amd import evaluator as evaluator_mod, sharding
    n = cfg["n_queries"]
    ev = evaluator_mod.Evaluator([[0]] * n, [[0]] * n, 4, "cpu")
    ev.filter, ev.use_seeds, ev.use_graph, ev.optimistic = cfg["filter"], cfg["use_seeds"], True, True
    ev._c_scalar(0.0)                              # (its device scalar, while the device is still the CPU)
    ev.device = torch.device("cuda")
    step, launches = {}, []
    ev._has_seeds = lambda K, n_items, branch=None: step["script"]["has_seeds"]
    ev._means_launch = launch_stub(ev, step, launches)
    saved = torch.cuda.current_stream, torch.cuda.Event, sharding.world
    torch.cuda.current_stream, torch.cuda.Event = (lambda *a: _Stream()), _Event
    tab = torch.zeros(4, 2)
    out = []
    try:
        for rec in cfg["evals"]:
            s = rec[0]
            step["script"] = s
            del launches[:]
            sharding.world = lambda: (0, s["world"])
            ev.use_graph = s["use_graph"]
            if s.get("seed_skip0"):
                ev._seed_skip = 0
            ev.test_mf(1, tab, None, tab, [20], tab[0], tab[0], 30.0)
            assert ev.use_graph == (s["use_graph"] and not s.get("graph_off"))
            out.append([s, [list(l) for l in launches], ev.last_eval_info(), [getattr(ev, k) for k in COUNTERS]])
    finally:
        torch.cuda.current_stream, torch.cuda.Event, sharding.world = saved
    return out


def record_policy():
    configs = []
    for k, (filt, n_queries, use_seeds) in enumerate(CONFIGS):
        cfg = {"filter": filt, "n_queries": n_queries, "use_seeds": use_seeds, "evals": [[s] for s in make_script(100 + k)]}
        cfg["evals"] = drive(cfg)
        assert len(cfg["evals"]) >= 200
        assert unpack(pack(cfg)) == cfg
        configs.append(cfg)
    # a trace that never leaves the happy path pins nothing: every back-off climbs to 16 and later returns to 1
    for col in (1, 3, 5):
        assert any(_climbs_and_returns([e[3][col] for e in cfg["evals"]]) for cfg in configs), COUNTERS[col]
    paths = {(bool(e[2].get("filter")), e[0]["world"]) for cfg in configs for e in cfg["evals"]}
    assert paths == {(True, 1), (False, 1), (False, 2)}, paths
    return [pack(cfg) for cfg in configs]


def _climbs_and_returns(values):
    return 16 in values and 1 in values[values.index(16):]


def pack(cfg):
    """{..., "evals": [[script, launches, info, counters], ...]} -> the file's form: a list per field"""
    evals = cfg["evals"]
    assert all(len({(l[1], l[2]) for l in e[1]}) == 1 for e in evals)      # (the launches of an evaluation differ in mode only)
    code = {tuple(v): k for k, v in MODES.items()}
    out = {k: v for k, v in cfg.items() if k != "evals"}
    out["script"] = {k: [int(e[0][k]) for e in evals] for k in SCRIPT}
    out["script"].update({k: [n for n, e in enumerate(evals) if e[0].get(k)] for k in ("graph_off", "seed_skip0")})
    out["launches"] = {"modes": [code[tuple(l[0] for l in e[1])] for e in evals], "seeded": [int(e[1][0][1]) for e in evals],
                       "filter": [e[1][0][2] for e in evals]}
    out["info"] = {k: [e[2].get(k) if k == "filter" else int(e[2][k]) for e in evals] for k in INFO}
    out["counters"] = {k: [e[3][n] for e in evals] for n, k in enumerate(COUNTERS)}
    return out


def unpack(packed):
    """the inverse of pack"""
    evals = []
    for n in range(len(packed["info"]["seeded"])):
        script = {k: packed["script"][k][n] for k in ("relisted", "exact_fallback", "world")}
        script.update({k: bool(packed["script"][k][n]) for k in ("has_seeds", "use_graph")})
        script.update({k: True for k in ("graph_off", "seed_skip0") if n in packed["script"][k]})
        la = packed["launches"]
        launches = [[mode, bool(la["seeded"][n]), la["filter"][n]] for mode in MODES[la["modes"][n]]]
        info = {k: packed["info"][k][n] for k in INFO}
        info.update(seeded=bool(info["seeded"]), redone=bool(info["redone"]))
        if info["filter"] is None:
            del info["filter"]
        evals.append([script, launches, info, [packed["counters"][k][n] for k in COUNTERS]])
    return dict({k: packed[k] for k in ("filter", "n_queries", "use_seeds")}, evals=evals)


# ----------------------------------------------------------------------------- kernel names (GPU)
def kernel_name_cases():
    return [(flavour, kind, filt) for flavour in ("mf", "lgcn") for kind in ("SCORE_NORMAL", "SCORE_RUBI_BOTH")
            for filt in ("f32", "f16")]


def kernel_names(flavour, kind, filt):
    """[names of an unseeded evaluation, names of the seeded one after it] at U=513, N=20011, d=128, launched directly"""
    import numpy as np
    from macr_amd import ops
    from macr_amd.evaluator import Evaluator
    rs = np.random.RandomState(141 + 513)
    U, N, d = 513, 20011, 128
    dev = lambda a: torch.from_numpy(a).cuda()
    P = dev((rs.standard_normal((U + 50, d)) * 0.4).astype(np.float32))
    Q = dev((rs.standard_normal((N, d)) * 0.4).astype(np.float32))
    w, wu = dev((rs.standard_normal(d) * 0.3).astype(np.float32)), dev((rs.standard_normal(d) * 0.3).astype(np.float32))
    uid = dev(rs.permutation(U + 50)[:U].astype(np.int32))
    mask = [sorted(rs.choice(N, 30, replace=False).tolist()) for _ in range(U)]
    gt = [sorted(rs.choice(N, 5, replace=False).tolist()) for _ in range(U)]
    ev = Evaluator(mask, gt, N, torch.device("cuda"))
    ev.filter, ev.use_graph, ev.use_seeds = filt, False, True
    assert ev._shape_uses_seeds(N, d)
    test = ev.test_mf if flavour == "mf" else ev.test_lgcn
    out = []
    for want_seeded in (False, True):
        ops.timing_begin()
        test(getattr(ops, kind), P, uid, Q, [20], w, wu, 1.0)
        out.append([name for name, _ in ops.timing_end()])
        assert ev.last_eval_info()["seeded"] is want_seeded
    return out


def record_kernel_names():
    return {"%s/%s/%s" % case: kernel_names(*case) for case in kernel_name_cases()}


if __name__ == "__main__":
    doc = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    if "--gpu" in sys.argv[1:]:
        doc["kernel_names"] = record_kernel_names()
    else:
        doc["policy"] = record_policy()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    with open(out, "w") as f:          # one line per list
        text = json.dumps(doc, sort_keys=True, indent=1, separators=(",", ": "))
        f.write(re.sub(r"\[[^\[\]{}]*\]", lambda m: json.dumps(json.loads(m.group(0)), separators=(",", ":")), text) + "\n")
    print("wrote", out)
