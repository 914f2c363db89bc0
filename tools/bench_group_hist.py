#!/usr/bin/env python3
"""Time of the per-row group histogram of MACR_CALIBRATION_REPORT (macr_group_hist: one launch) beside k_metrics_mf, which reads
the same rankings and ground-truth lists, with the library's own per-kernel timing (macr_timing_*: a hipEvent after every
launch), warmed up, the calls alternating in one process, median of the repeats.  Two shapes:
    gowalla   the Gowalla evaluation shape, 15 424 users x k = 20 over 40 981 items: the corrected (rubi_both, c = 40) ranking of
              an MF model trained for a few epochs on macr_amd/synth.py's Gowalla-shaped workload, and its train lists
    zipf      2^20 users x k = 20 over 10^6 items: tools/bench_item_counts.py's Zipf rankings, and as train lists rows of
              0 .. 63 Zipf items (timing only)
Two calls are timed at each: the ranking form (cnt, hit, wsum on the lists, with the ground truth) and the CSR form on the train
lists (cnt, wsum: what the evaluator computes once and keeps).  The ranking form is held to 2x the measured k_metrics_mf time:
the same reads plus one gather per entry.  The CSR form reads other data (the train lists, several times the entries of the
lists); its time is recorded beside the same yardstick, with its entries, and has no bound.
Usage: python tools/bench_group_hist.py [--repeats 50] [--epochs 3] [--out FILE]  -> a few lines of text and one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402
from bench_item_counts import zipf  # noqa: E402  (tools/ is this script's directory)
from bench_list_shift import gowalla  # noqa: E402

K = 20
G = 6


def measure(rankings, train, gt, n_items, group_of, weight, repeats, warmup=10):
    """median microseconds per call over `repeats` timed rounds of the three calls, each call in a timing window of its own"""
    seen = {}
    calls = (("group_hist_ranking", lambda: ops.group_hist(rankings, group_of, G, n_items, k=K, gt=gt, item_weight=weight)),
             ("group_hist_csr", lambda: ops.group_hist(train, group_of, G, n_items, item_weight=weight)),
             ("metrics_mf", lambda: ops.metrics_mf(rankings, None, gt, [K])))
    for r in range(warmup + repeats):
        for label, call in calls:
            ops.timing_begin()
            call()
            kernel = "metrics_mf" if label == "metrics_mf" else "group_hist"
            ms = [t for name, t in ops.timing_end() if name == kernel]
            assert len(ms) == 1, (label, ms)
            if r >= warmup:
                seen.setdefault(label, []).append(1e3 * ms[0])
    return {name: float(np.median(v)) for name, v in seen.items()}


def zipf_train_lists(dev, U, n_items):
    """a CSR of U rows of 0 .. 63 Zipf items"""
    gen = torch.Generator(device=dev).manual_seed(7)
    lengths = torch.randint(0, 64, (U,), generator=gen, device=dev, dtype=torch.int64)
    ptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(lengths, 0)
    nnz = int(ptr[-1])
    cdf = synth.zipf_cdf(n_items, dev)
    relabel = torch.randperm(n_items, generator=gen, device=dev).to(torch.int32)
    r = torch.rand(nnz, generator=gen, device=dev, dtype=torch.float64)
    idx = relabel[torch.searchsorted(cdf, r, right=True).clamp_(max=n_items - 1)].contiguous()
    return ops.CSR(ptr.to(torch.int32), idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "k": K}
    lines = ["macr_group_hist beside k_metrics_mf, %s, median of %d, microseconds" % (res["device"], a.repeats)]

    ev, args, (w, wu, c), group_np = gowalla(dev, a.epochs)
    _, here, _ = ev.rank(*args, K, w, wu, c)
    zb, zgt, zn, zgroup = zipf(dev)
    shapes = (("gowalla", (here, ev.mask, ev.gt, ev.n_items, group_np)),
              ("zipf", (zb, zipf_train_lists(dev, zb.shape[0], zn), zgt, zn, zgroup)))
    for name, (rankings, train, gt, n_items, groups) in shapes:
        group_of = torch.from_numpy(np.asarray(groups, dtype=np.int32)).to(dev)
        weight = torch.randint(0, 5000, (n_items,), generator=torch.Generator(device=dev).manual_seed(9), device=dev, dtype=torch.int32)
        cnt, hit, wsum = ops.group_hist(rankings, group_of, G, n_items, k=K, gt=gt, item_weight=weight)
        p_cnt, _, p_wsum = ops.group_hist(train, group_of, G, n_items, item_weight=weight)
        med = measure(rankings, train, gt, n_items, group_of, weight, a.repeats)
        ratio, ratio_csr = med["group_hist_ranking"] / med["metrics_mf"], med["group_hist_csr"] / med["metrics_mf"]
        entries, train_entries = int(wsum[:, 1].sum()), int(p_wsum[:, 1].sum())
        res[name] = dict(users=rankings.shape[0], n_items=n_items, list_entries=entries, hits=int(hit.sum()), train_entries=train_entries,
                         ratio=round(ratio, 3), within_2x=bool(ratio <= 2.0), ratio_csr=round(ratio_csr, 3),
                         **{k: round(v, 2) for k, v in med.items()})
        lines.append("%-8s %8d users x %d over %8d items: group_hist on the lists %.1f   metrics_mf %.1f   ratio %.2f: 2x bound %s   |   "
                     "group_hist on the train lists (%d entries against %d, no bound) %.1f   ratio %.2f" % (
                         name, rankings.shape[0], K, n_items, med["group_hist_ranking"], med["metrics_mf"], ratio,
                         "met" if ratio <= 2.0 else "MISSED", train_entries, entries, med["group_hist_csr"], ratio_csr))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
