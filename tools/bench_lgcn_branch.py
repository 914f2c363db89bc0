#!/usr/bin/env python3
"""LightGCN's item-branch losses and rankings against the two-branch ones, Yelp2018 shape (B = 4096, d = 64, 2 layers):
    step        --loss bce1 (MACR_LOSS_RUBIBCE), --loss bce2 (MACR_LOSS_RUBIBCE_EGO) vs --loss bceboth (HIP events around N steps)
    evaluation  --test rubi1, rubi2 vs rubiboth: Evaluator.test_lgcn at c = 40, Ks = [20], every user (wall clock per call;
                each call returns its means to the host, as the CLI's does)
Kinds alternate in rounds so that clock drift hits all alike.
Usage: python tools/bench_lgcn_branch.py [--steps 200] [--evals 20] [--rounds 5] [--out profiles/lgcn_item_branch.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402
from macr_amd.evaluator import Evaluator  # noqa: E402


def timed_steps(state, kind, batches, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(n):
        b = batches[k % batches.shape[0]]
        state.step(kind, b[0], b[1], b[2])
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / n


def timed_evals(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    return 1e6 * (time.perf_counter() - t0) / n


def summary(us, base):
    out = {k: [round(x, 2) for x in v] for k, v in us.items()}
    out.update({"%s_over_%s_median" % (k, base): round(float(np.median(v) / np.median(us[base])), 4) for k, v in us.items() if k != base})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lgcn_item_branch.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"steps_per_round": a.steps, "evals_per_round": a.evals, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    cfg = synth.WORKLOADS["yelp2018"]
    n_u, n_i, d, B, L = cfg["n_users"], cfg["n_items"], 64, 4096, 2
    lists = synth.interaction_lists(n_u, n_i, cfg["n_train"] / n_u, seed=9)
    rows = np.repeat(np.arange(n_u), [len(x) for x in lists])
    R = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, np.concatenate(lists))), shape=(n_u, n_i))
    A = sp.bmat([[None, R], [R.T, None]], format="csr", dtype=np.float32)
    deg = np.asarray(A.sum(1)).ravel()
    with np.errstate(divide="ignore"):
        dinv = np.power(deg, -0.5).astype(np.float32)
    dinv[np.isinf(dinv)] = 0
    A = (sp.diags(dinv) @ A @ sp.diags(dinv)).tocsr().astype(np.float32)
    A.sort_indices()
    adj = ops.CSR.from_scipy(A, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    T = synth.xavier_table(n_u + n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    hyper = ops.make_hyper(1e-3, 1e-5, cfg["alpha"], cfg["beta"], B)
    names = {"bceboth": ops.LOSS_RUBIBCEBOTH, "bce1": ops.LOSS_RUBIBCE, "bce2": ops.LOSS_RUBIBCE_EGO}
    states = {k: ops.LGCNState(T.clone(), n_u, n_i, w.clone(), w.clone(), adj, L, hyper, B) for k in names}
    batches = synth.train_batches(32, n_u, n_i, B, gen, dev)
    for k, kind in names.items():                         # warm-up: workspaces, first-touch, clocks
        timed_steps(states[k], kind, batches, 20)
    us = {k: [] for k in names}
    for _ in range(a.rounds):
        for k, kind in names.items():
            us[k].append(timed_steps(states[k], kind, batches, a.steps))
    out["step_yelp2018_us"] = summary(us, "bceboth")

    # evaluation on the trained bceboth tables: every user against every item, train items masked
    st = states["bceboth"]
    E = st.propagated()
    ua, ia = E[:n_u], E[n_u:].contiguous()
    ego = st.T[n_u:]
    rs = np.random.RandomState(3)
    gt = [sorted(set(rs.randint(0, n_i, 5).tolist())) for _ in range(n_u)]
    ev = Evaluator([list(x) for x in lists], gt, n_i, dev)
    uid = torch.arange(n_u, dtype=torch.int32, device=dev)
    runs = {"rubiboth": lambda: ev.test_lgcn(ops.SCORE_RUBI_BOTH, ua, uid, ia, [20], st.w, st.wu, 40.0),
            "rubi1": lambda: ev.test_lgcn(ops.SCORE_RUBI, ua, uid, ia, [20], st.w, st.wu, 40.0),
            "rubi2": lambda: ev.test_lgcn(ops.SCORE_RUBI, ua, uid, ia, [20], st.w, st.wu, 40.0, branch=ego)}
    for r in runs.values():
        timed_evals(r, 3)
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, r in runs.items():
            us[k].append(timed_evals(r, a.evals))
    out["eval_yelp2018_us"] = summary(us, "rubi1")
    out["eval_yelp2018_us"]["rubiboth_over_rubi1_median"] = round(float(np.median(us["rubiboth"]) / np.median(us["rubi1"])), 4)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
