#!/usr/bin/env python3
"""Time of the position-weighted exposure kernels (macr_item_exposure: exposure_zero + item_exposure + exposure_finish) beside
the per-item counting kernels (macr_item_counts: item_zero + item_counts + item_finish) on the same rankings and ground-truth
lists, with the library's own per-kernel timing (macr_timing_*: a hipEvent after every launch), warmed up, the two calls
alternating in one process, median of the repeats.  The two shapes of tools/bench_item_counts.py (its builders are imported):
    gowalla   15 424 users x k = 20 over 40 981 items, the rankings of a briefly trained MF model
    zipf      2^20 users x k = 20 over 10^6 items with a Zipf head
The new call is held to 2x the measured macr_item_counts call at both shapes: it does up to two 64-bit LDS adds per entry
where the yardstick does one, and its counter copies are twice as wide.
Usage: python tools/bench_item_exposure.py [--repeats 50] [--epochs 3] [--out FILE]  -> a few lines of text and one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import exposure, ops  # noqa: E402
from bench_item_counts import gowalla, zipf  # noqa: E402  (tools/ is this script's directory)

COUNT_KERNELS = ("item_zero", "item_counts", "item_finish")
EXPOSURE_KERNELS = ("exposure_zero", "item_exposure", "exposure_finish")


def measure(rankings, gt, weights, n_items, group_of, repeats, warmup=10):
    """median microseconds per kernel name over `repeats` timed pairs of calls; each call in a timing window of its own, so
    that both sides' first kernel stands behind the same window start"""
    k = len(weights)
    seen = {}
    for r in range(warmup + repeats):
        for call in (lambda: ops.item_exposure(rankings, gt, weights, n_items, group_of, 6),
                     lambda: ops.item_counts(rankings, gt, k, n_items, group_of, 6)):
            ops.timing_begin()
            call()
            for name, ms in ops.timing_end():
                if r >= warmup:
                    seen.setdefault(name, []).append(1e3 * ms)
    med = {name: float(np.median(v)) for name, v in seen.items()}
    med["counts_total"] = sum(med[n] for n in COUNT_KERNELS)
    med["exposure_total"] = sum(med[n] for n in EXPOSURE_KERNELS)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    weights = exposure.position_weights(20)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "k": 20}
    lines = ["macr_item_exposure beside macr_item_counts, %s, median of %d, microseconds" % (res["device"], a.repeats)]
    for name, make in (("gowalla", lambda: gowalla(dev, a.epochs)), ("zipf", lambda: zipf(dev))):
        rankings, gt, n_items, group_np = make()
        group_of = torch.from_numpy(group_np).to(dev)
        exp_w, hit_w, sums = ops.item_exposure(rankings, gt, weights, n_items, group_of, 6)
        rec, hit, _ = ops.item_counts(rankings, gt, 20, n_items, group_of, 6)
        ones, ones_hit, _ = ops.item_exposure(rankings, gt, np.ones(20, dtype=np.uint32), n_items, group_of, 6)
        assert torch.equal(ones, rec.long()) and torch.equal(ones_hit, hit.long())         # the two calls count the same entries
        med = measure(rankings, gt, weights, n_items, group_of, a.repeats)
        ratio = med["exposure_total"] / med["counts_total"]
        res[name] = dict(users=rankings.shape[0], n_items=n_items, slots=int(rec.sum()), hits=int(hit.sum()),
                         exposure_sum=int(exp_w.sum()), ratio=round(ratio, 3), within_2x=bool(ratio <= 2.0),
                         **{k: round(v, 2) for k, v in med.items()})
        lines.append("%-8s %8d users x 20 over %8d items: exposure_zero %.1f + item_exposure %.1f + exposure_finish %.1f = %.1f   "
                     "item_zero %.1f + item_counts %.1f + item_finish %.1f = %.1f   ratio %.2f: 2x bound %s" % (
                         name, rankings.shape[0], n_items, med["exposure_zero"], med["item_exposure"], med["exposure_finish"],
                         med["exposure_total"], med["item_zero"], med["item_counts"], med["item_finish"], med["counts_total"],
                         ratio, "met" if ratio <= 2.0 else "MISSED"))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
