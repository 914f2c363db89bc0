#!/usr/bin/env python3
"""Time of the full-catalogue position count (macr_rank_positions: rank_keys + rank_cols + rank_count + rank_finish) beside the
ranking kernels of an fp32-filter evaluation (MACR_EVAL_FILTER=f32: score_sample + tau + score_stream + select), which do the
same U x N x d fp32 products on the same tile, with the library's own per-kernel timing (macr_timing_*: a hipEvent after every
launch), warmed up, median of the repeats, each call in a timing window of its own.

Shape: the Gowalla evaluation shape, 15 424 query users x 40 981 items, d = 64, the tables of an MF model trained for a few
epochs on macr_amd/synth.py's Gowalla-shaped workload, scored as rubi_both at c = 40; masks and ground truth are
synth.eval_problem's (what tools/bench_item_counts.py ranks): 13 held-out items per user.  A second set of pair lists with the
same users and about the same number of pairs but lognormal lengths shows what long lists cost (a list is cut into columns
of 16 pairs).

The counting call is held to 2x the evaluation's ranking kernels.  To take the bound from another build (the parent commit's):
run a copy of this file inside that checkout with --only-eval --label parent --out base.json (that mode uses nothing the
parent lacks) and pass --baseline base.json to the full run here.

Usage: python tools/bench_rank_positions.py [--repeats 50] [--epochs 3] [--only-eval] [--label NAME] [--baseline FILE] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402
from macr_amd.evaluator import Evaluator  # noqa: E402

RANK_KERNELS = ("rank_keys", "rank_cols", "rank_count", "rank_finish")
EVAL_KERNELS = ("score_sample", "tau", "score_stream", "select")         # (the sampling pass by its prefix: score_sample_b is the fp16 one)
KIND, C = ops.SCORE_RUBI_BOTH, 40.0


def medians(call, repeats, warmup=10):
    """median microseconds per kernel name of `call`, each call in a timing window of its own"""
    seen = {}
    for r in range(warmup + repeats):
        ops.timing_begin()
        call()
        for name, ms in ops.timing_end():
            if r >= warmup:
                seen.setdefault(name, []).append(1e3 * ms)
    return {name: float(np.median(v)) for name, v in seen.items()}


def ranking_sum(per_kernel):
    """the first round's ranking kernels of an evaluation: sampling pass (whichever it is), tau, listing pass, selection"""
    return sum(v for k, v in per_kernel.items() if not k.endswith("2") and (k.startswith("score_sample") or k in EVAL_KERNELS[1:]))


def model(dev, epochs):
    cfg = synth.WORKLOADS["gowalla"]
    n_u, n_i, d, B = cfg["n_users"], cfg["n_items"], cfg["d"], cfg["batch"]
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w, wu = synth.xavier_table(d, 1, gen, dev).reshape(-1), synth.xavier_table(d, 1, gen, dev).reshape(-1)
    state = ops.MFState(P, Q, w, wu, ops.make_hyper(1e-3, 1e-5, cfg["alpha"], cfg["beta"], B), B)
    batches = synth.train_batches(cfg["n_train"] // B + 1, n_u, n_i, B, gen, dev)
    for _ in range(epochs):
        for b in batches:
            state.step(ops.LOSS_RUBIBCEBOTH, b[0], b[1], b[2])
    return cfg, state


def skewed_lists(mask, n_items, total, seed=5):
    """ground-truth lists of lognormal length (sigma 1.2, clipped to [1, 2000]) adding up to about `total` pairs"""
    rs = np.random.RandomState(seed)
    lens = rs.lognormal(0.0, 1.2, len(mask))
    lens = np.clip(np.round(lens * total / lens.sum()), 1, 2000).astype(np.int64)
    return [sorted(set(rs.randint(0, n_items, int(n)).tolist()) - set(row)) for n, row in zip(lens, mask)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--only-eval", action="store_true", help="time the fp32-filter evaluation only and write its JSON")
    ap.add_argument("--label", default="this build", help="how the report names the build that ran the evaluation")
    ap.add_argument("--baseline", default=None, help="JSON of an --only-eval run of another build: the bound comes from it")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, state = model(dev, a.epochs)
    users, mask, gt = synth.eval_problem(cfg, seed=3)
    uid = torch.from_numpy(users).to(dev)
    n_i = cfg["n_items"]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "users": len(users), "n_items": n_i, "d": cfg["d"],
           "lib": a.label}

    ev = Evaluator(mask, gt, n_i, dev)
    ev.use_graph = ev.use_seeds = False               # every launch under the timer, the sampling pass every time
    ev_med = medians(lambda: ev.rank_local(KIND, state.P, uid, state.Q, 20, state.w, state.wu, C, seeded=False, filter="f32"),
                     a.repeats)
    res["eval_f32"] = {k: round(v, 2) for k, v in ev_med.items()}
    res["eval_f32_ranking"] = round(ranking_sum(ev_med), 2)
    lines = ["fp32-filter evaluation (%s), %s, median of %d, microseconds: %s; ranking kernels %s = %.1f" % (
        res["lib"], res["device"], a.repeats, "  ".join("%s %.1f" % kv for kv in ev_med.items()), " + ".join(EVAL_KERNELS),
        res["eval_f32_ranking"])]
    if not a.only_eval:
        base = json.load(open(a.baseline)) if a.baseline else res
        base["eval_f32_ranking"] = round(ranking_sum(base["eval_f32"]), 2)
        bound = 2 * base["eval_f32_ranking"]
        sig_i, sig_u = ops.branch_sigmoid2(state.Q, state.w, None, state.P, state.wu, uid)
        for name, lists in (("gowalla", gt), ("skewed", skewed_lists(mask, n_i, sum(len(r) for r in gt)))):
            pairs = ops.CSR.from_lists(lists, dev)
            lens = np.asarray([len(r) for r in lists])
            call = lambda: ops.rank_positions(KIND, state.P, uid, state.Q, pairs, sig_u, sig_i, C, ev.mask, n_pairs=int(lens.sum()))
            pos = call().cpu().numpy()
            med = medians(call, a.repeats)
            total = sum(med[k] for k in RANK_KERNELS)
            res[name] = dict(pairs=int(lens.sum()), mean_len=round(float(lens.mean()), 2), max_len=int(lens.max()),
                             columns=int(((lens + 15) // 16).sum()), median_position=float(np.median(pos[pos >= 0])),
                             no_position=int((pos < 0).sum()), total=round(total, 2), **{k: round(med[k], 2) for k in RANK_KERNELS})
            lines.append("%-8s %d users x %d items, d = %d; %d pairs (mean %.1f, max %d per user, %d columns of <= 16): "
                         "rank_keys %.1f + rank_cols %.1f + rank_count %.1f + rank_finish %.1f = %.1f" % (
                             name, len(users), n_i, cfg["d"], lens.sum(), lens.mean(), lens.max(), res[name]["columns"],
                             med["rank_keys"], med["rank_cols"], med["rank_count"], med["rank_finish"], total))
        g = res["gowalla"]
        res["bound"] = round(bound, 2)
        res["bound_from"] = base["lib"]
        res["gowalla_call_within_2x_eval_f32"] = bool(g["total"] <= bound)
        lines.append("bound 2 x the fp32-filter evaluation's ranking kernels (%s: %.1f, of which score_stream %.1f) = %.1f at the "
                     "Gowalla shape: the counting call %.1f (%s)" % (base["lib"], base["eval_f32_ranking"], base["eval_f32"]["score_stream"],
                                                                       bound, g["total"], "met" if g["total"] <= bound else "MISSED"))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n" if a.only_eval else text)


if __name__ == "__main__":
    main()
