#!/usr/bin/env python3
"""Time of the list comparison kernel of MACR_SHIFT_REPORT (macr_list_shift: one launch) beside k_metrics_mf, which reads the
same rankings and ground-truth lists, with the library's own per-kernel timing (macr_timing_*: a hipEvent after every launch),
warmed up, the two calls alternating in one process, median of the repeats.  Two shapes:
    gowalla   the Gowalla evaluation shape, 15 424 users x k = 20 over 40 981 items: the factual (normal) and the corrected
              (rubi_both, c = 40) rankings of an MF model trained for a few epochs on macr_amd/synth.py's Gowalla-shaped workload
    zipf      2^20 users x k = 20 over 10^6 items: tools/bench_item_counts.py's Zipf rankings as the base, and as `here` the same
              rows rotated by one slot with every other column drawn anew (a list may repeat an id: timing only)
The kernel is held to 2x the measured k_metrics_mf time at both shapes: it reads two rankings and writes two lists plus 32 bytes
per query where metrics_mf reads one ranking.  At the Gowalla shape the whole MACR_SHIFT_REPORT=1 call (Evaluator.list_shift: two
rankings, list_shift, two item_counts) and the =2 call (+ Evaluator.shift_depth) are timed too, by the wall clock around a
synchronised call, median of the repeats; they have no bound.
Usage: python tools/bench_list_shift.py [--repeats 50] [--epochs 3] [--out FILE]  -> a few lines of text and one JSON line"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, popularity, synth  # noqa: E402
from macr_amd.evaluator import Evaluator  # noqa: E402
from bench_item_counts import zipf  # noqa: E402  (tools/ is this script's directory)

K, C = 20, 40.0


def measure(base, here, gt, n_items, repeats, warmup=10):
    """median microseconds per kernel name over `repeats` timed pairs of calls, each call in a timing window of its own"""
    out = tuple(torch.empty(s, dtype=torch.int32, device=base.device) for s in ((base.shape[0], 8), (base.shape[0], K), (base.shape[0], K)))
    seen = {}
    for r in range(warmup + repeats):
        for call in (lambda: ops.list_shift(base, here, gt, K, n_items, out=out),
                     lambda: ops.metrics_mf(here, None, gt, [K])):
            ops.timing_begin()
            call()
            for name, ms in ops.timing_end():
                if r >= warmup:
                    seen.setdefault(name, []).append(1e3 * ms)
    return {name: float(np.median(v)) for name, v in seen.items()}


def wall(call, repeats, warmup=5):
    """median microseconds of a synchronised call"""
    t = []
    for r in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if r >= warmup:
            t.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(t))


def gowalla(dev, epochs):
    """-> (evaluator, the arguments of Evaluator.list_shift, group ids) of a briefly trained two-branch MF model"""
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
    users, mask, gt = synth.eval_problem(cfg, seed=3)
    ev = Evaluator(mask, gt, n_i, dev)
    train_counts = np.bincount(batches[:, 1].reshape(-1).cpu().numpy(), minlength=n_i)
    args = (ops.SCORE_RUBI_BOTH, state.P, torch.from_numpy(users).to(dev), state.Q)
    return ev, args, (state.w, state.wu, C), popularity.item_groups(train_counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "k": K}
    lines = ["macr_list_shift beside k_metrics_mf, %s, median of %d, microseconds" % (res["device"], a.repeats)]

    ev, args, (w, wu, c), group_np = gowalla(dev, a.epochs)
    _, here, _ = ev.rank(*args, K, w, wu, c)
    _, base, _ = ev._base_evaluator().rank(ops.SCORE_NORMAL, *args[1:], K)
    zb, zgt, zn, _ = zipf(dev)
    zh = torch.roll(zb, 1, dims=1)
    zh[:, ::2] = torch.randint(0, zn, zh[:, ::2].shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev, dtype=torch.int32)
    for name, (b, h, gt, n_items) in (("gowalla", (base, here, ev.gt, ev.n_items)), ("zipf", (zb, zh.contiguous(), zgt, zn))):
        pu, ent, left = ops.list_shift(b, h, gt, K, n_items)
        tot = pu.long().sum(0).tolist()
        med = measure(b, h, gt, n_items, a.repeats)
        ratio = med["list_shift"] / med["metrics_mf"]
        res[name] = dict(users=b.shape[0], n_items=n_items, common=tot[2], n_here=tot[1], entered=int((ent >= 0).sum()),
                         identical=int((pu[:, 3] == K).sum()), ratio=round(ratio, 3), within_2x=bool(ratio <= 2.0),
                         **{k: round(v, 2) for k, v in med.items()})
        lines.append("%-8s %8d users x %d over %8d items (overlap %.3f): list_shift %.1f   metrics_mf %.1f   ratio %.2f: 2x bound %s" % (
            name, b.shape[0], K, n_items, tot[2] / max(tot[1], 1), med["list_shift"], med["metrics_mf"], ratio,
            "met" if ratio <= 2.0 else "MISSED"))

    shift = lambda: ev.list_shift(*args, K, w, wu, c, group_of=group_np, n_groups=6)
    _, ent, left, _, _ = shift()
    call_1 = wall(shift, a.repeats)
    call_2 = wall(lambda: ev.shift_depth(*args, *shift()[1:3], w, wu, c), a.repeats)
    evaluation = wall(lambda: ev.test_mf(*args, [K], w, wu, c), a.repeats)
    res["gowalla_calls"] = dict(value_1=round(call_1, 1), value_2=round(call_2, 1), evaluation=round(evaluation, 1))
    lines.append("gowalla, whole calls by the wall clock (no bound): MACR_SHIFT_REPORT=1 (two rankings, list_shift, two item_counts) %.0f   "
                 "=2 (+ the positions of %d entered and %d left items) %.0f   one evaluation (test_mf) %.0f" % (
                     call_1, int((ent >= 0).sum()), int((left >= 0).sum()), call_2, evaluation))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
