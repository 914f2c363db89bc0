#!/usr/bin/env python3
"""Time of the per-item counting kernels (macr_item_counts: item_zero + item_counts + item_finish) beside k_metrics_mf, which
reads the same rankings and ground-truth lists, with the library's own per-kernel timing (macr_timing_*: a hipEvent after
every launch), warmed up, median of the repeats.  Two shapes:
    gowalla   the Gowalla evaluation shape, 15 424 users x k = 20 over 40 981 items: the rankings of an MF model trained for a
              few epochs on macr_amd/synth.py's Gowalla-shaped workload (Zipf positives, so the lists have a popular head)
    zipf      2^20 users x k = 20 over 10^6 items, ids drawn from Zipf(1.0) over a shuffled catalogue (a list may repeat an
              id: timing only), 8 ground-truth ids per user
The counting kernels are held to 2x the measured k_metrics_mf time at the Gowalla shape (the extra factor is for the scatter).
Usage: python tools/bench_item_counts.py [--repeats 50] [--epochs 3] [--out FILE]  -> a few lines of text and one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, popularity, synth  # noqa: E402
from macr_amd.evaluator import Evaluator  # noqa: E402

ITEM_KERNELS = ("item_zero", "item_counts", "item_finish")


def measure(rankings, gt, k, n_items, group_of, repeats, warmup=10):
    """median microseconds per kernel name over `repeats` timed pairs of calls; each call in a timing window of its own, so
    that both sides' first kernel stands behind the same window start"""
    seen = {}
    for r in range(warmup + repeats):
        for call in (lambda: ops.item_counts(rankings, gt, k, n_items, group_of, 6),
                     lambda: ops.metrics_mf(rankings, None, gt, [k])):
            ops.timing_begin()
            call()
            for name, ms in ops.timing_end():
                if r >= warmup:
                    seen.setdefault(name, []).append(1e3 * ms)
    med = {name: float(np.median(v)) for name, v in seen.items()}
    med["item_total"] = sum(med[n] for n in ITEM_KERNELS)
    return med


def gowalla(dev, epochs):
    cfg = synth.WORKLOADS["gowalla"]
    n_u, n_i, d, B = cfg["n_users"], cfg["n_items"], cfg["d"], cfg["batch"]
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    state = ops.MFState(P, Q, w, w.clone(), ops.make_hyper(1e-3, 1e-5, cfg["alpha"], cfg["beta"], B), B)
    n_batch = cfg["n_train"] // B + 1
    batches = synth.train_batches(n_batch, n_u, n_i, B, gen, dev)
    for _ in range(epochs):
        for b in batches:
            state.step(ops.LOSS_NORMALBCE, b[0], b[1], b[2])
    users, mask, gt = synth.eval_problem(cfg, seed=3)
    ev = Evaluator(mask, gt, n_i, dev)
    _, idx, _ = ev.rank(ops.SCORE_NORMAL, state.P, torch.from_numpy(users).to(dev), state.Q, 20)
    train_counts = np.bincount(batches[:, 1].reshape(-1).cpu().numpy(), minlength=n_i)
    return idx, ev.gt, n_i, popularity.item_groups(train_counts)


def zipf(dev, U=1 << 20, n_items=1000000, K=20, n_gt=8):
    gen = torch.Generator(device=dev).manual_seed(2)
    cdf = synth.zipf_cdf(n_items, dev)
    relabel = torch.randperm(n_items, generator=gen, device=dev).to(torch.int32)
    r = torch.rand((U, K), generator=gen, device=dev, dtype=torch.float64)
    rankings = relabel[torch.searchsorted(cdf, r, right=True).clamp_(max=n_items - 1)].contiguous()
    truth = torch.sort(torch.randint(0, n_items, (U, n_gt), generator=gen, device=dev, dtype=torch.int32), dim=1).values
    truth[:, 0] = torch.minimum(truth[:, 0], rankings[:, 3])          # some hits; rows stay ascending
    gt = ops.CSR(torch.arange(0, (U + 1) * n_gt, n_gt, dtype=torch.int32, device=dev), truth.reshape(-1).contiguous())
    rank_of = torch.empty(n_items, dtype=torch.int64, device=dev)
    rank_of[relabel.long()] = torch.arange(n_items, device=dev)
    group_of = popularity.item_groups((5000.0 / (rank_of.cpu().numpy() + 1)).astype(np.int64))
    return rankings, gt, n_items, group_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "k": 20}
    lines = ["macr_item_counts beside k_metrics_mf, %s, median of %d, microseconds" % (res["device"], a.repeats)]
    for name, make in (("gowalla", lambda: gowalla(dev, a.epochs)), ("zipf", lambda: zipf(dev))):
        rankings, gt, n_items, group_np = make()
        group_of = torch.from_numpy(group_np).to(dev)
        rec, hit, sums = ops.item_counts(rankings, gt, 20, n_items, group_of, 6)
        med = measure(rankings, gt, 20, n_items, group_of, a.repeats)
        top = torch.sort(rec, descending=True).values[:1000].sum().item() / max(int(rec.sum()), 1)
        res[name] = dict(users=rankings.shape[0], n_items=n_items, slots=int(rec.sum()), hits=int(hit.sum()),
                         head1000_share=round(top, 4), **{k: round(v, 2) for k, v in med.items()})
        lines.append("%-8s %8d users x 20 over %8d items (1000 hottest items: %.1f %% of the slots): item_zero %.1f + item_counts %.1f "
                     "+ item_finish %.1f = %.1f   metrics_mf %.1f   ratio %.2f" % (
                         name, rankings.shape[0], n_items, 100 * top, med["item_zero"], med["item_counts"], med["item_finish"],
                         med["item_total"], med["metrics_mf"], med["item_total"] / med["metrics_mf"]))
    g = res["gowalla"]
    res["gowalla_kernel_within_2x_metrics_mf"] = bool(g["item_counts"] <= 2 * g["metrics_mf"])
    res["gowalla_call_within_2x_metrics_mf"] = bool(g["item_total"] <= 2 * g["metrics_mf"])
    lines.append("bound 2 x metrics_mf = %.1f at the Gowalla shape: the counting kernel %.1f (%s), the whole call's three launches %.1f (%s)" % (
        2 * g["metrics_mf"], g["item_counts"], "met" if res["gowalla_kernel_within_2x_metrics_mf"] else "MISSED",
        g["item_total"], "met" if res["gowalla_call_within_2x_metrics_mf"] else "MISSED"))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
