#!/usr/bin/env python3
"""Per-step time of the BPR losses against the BCE ones on the same shapes (HIP events around N steps, no host sync inside):
    MF        --train normal (MACR_LOSS_BPR)       vs --train normalbce   Gowalla shape, B = 4096, d = 64
    LightGCN  --loss bpr     (MACR_LOSS_BPR_LGCN)  vs --loss bce          Yelp2018 shape, B = 4096, d = 64, 2 layers
The bytes moved are the same for each pair of kinds (3 rows read, 3 gradient rows written per triple, the dense Adam pass);
only the per-pair epilogue differs.  Kinds alternate in rounds so that clock drift hits both alike.
Usage: python tools/bench_bpr.py [--steps 200] [--rounds 5]  -> one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402


def timed(step, batches, n):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(n):
        b = batches[k % batches.shape[0]]
        step(b[0], b[1], b[2])
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / n


def compare(name, steps, kinds, batches, n, rounds):
    for kind in kinds:                                    # warm-up: workspaces, first-touch, clocks
        timed(lambda u, i, j: steps[kind](kind, u, i, j), batches, 20)
    us = {k: [] for k in kinds}
    for _ in range(rounds):
        for kind in kinds:
            us[kind].append(timed(lambda u, i, j: steps[kind](kind, u, i, j), batches, n))
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"steps_per_round": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}

    cfg = synth.WORKLOADS["gowalla"]
    n_u, n_i, d, B = cfg["n_users"], cfg["n_items"], 64, 4096
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    hyper = ops.make_hyper(1e-3, 1e-5, cfg["alpha"], cfg["beta"], B)
    states = {k: ops.MFState(P.clone(), Q.clone(), w.clone(), w.clone(), hyper, B) for k in (ops.LOSS_BPR, ops.LOSS_NORMALBCE)}
    batches = synth.train_batches(32, n_u, n_i, B, gen, dev)
    steps = {k: (lambda kind, u, i, j, s=s: s.step(kind, u, i, j)) for k, s in states.items()}
    us = compare("mf", steps, (ops.LOSS_BPR, ops.LOSS_NORMALBCE), batches, a.steps, a.rounds)
    out["mf_gowalla"] = {"normal_us": [round(x, 2) for x in us[ops.LOSS_BPR]],
                         "normalbce_us": [round(x, 2) for x in us[ops.LOSS_NORMALBCE]],
                         "ratio_median": round(float(np.median(us[ops.LOSS_BPR]) / np.median(us[ops.LOSS_NORMALBCE])), 4)}

    cfg = synth.WORKLOADS["yelp2018"]
    n_u, n_i, B, L = cfg["n_users"], cfg["n_items"], 4096, 2
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
    T = synth.xavier_table(n_u + n_i, d, gen, dev)
    hyper = ops.make_hyper(1e-3, 1e-5, cfg["alpha"], cfg["beta"], B)
    states = {k: ops.LGCNState(T.clone(), n_u, n_i, w.clone(), w.clone(), adj, L, hyper, B)
              for k in (ops.LOSS_BPR_LGCN, ops.LOSS_NORMALBCE)}
    batches = synth.train_batches(32, n_u, n_i, B, gen, dev)
    steps = {k: (lambda kind, u, i, j, s=s: s.step(kind, u, i, j)) for k, s in states.items()}
    us = compare("lgcn", steps, (ops.LOSS_BPR_LGCN, ops.LOSS_NORMALBCE), batches, a.steps, a.rounds)
    out["lightgcn_yelp2018"] = {"bpr_us": [round(x, 2) for x in us[ops.LOSS_BPR_LGCN]],
                                "bce_us": [round(x, 2) for x in us[ops.LOSS_NORMALBCE]],
                                "ratio_median": round(float(np.median(us[ops.LOSS_BPR_LGCN]) / np.median(us[ops.LOSS_NORMALBCE])), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
