"""NumPy restatement of the position-weighted exposure count (macr_item_exposure) and of the report built on it
(macr_amd/exposure.py::summarize), written from their definitions and independent of both: plain loops and np.add.at on
int64, Python integers and fractions for the report."""
from fractions import Fraction

import numpy as np


def weights(k):
    """floor(2^24 / log2(p + 2) + 0.5) for p < k"""
    return np.floor(2.0 ** 24 / np.log2(np.arange(k, dtype=np.float64) + 2.0) + 0.5).astype(np.uint32)


def item_exposure(rankings, gt_lists, pos_weight, n_items):
    """(exp_w, hit_w) int64[n_items]: the sum of pos_weight[p] over the entries (u, p < len(pos_weight)) naming the item /
    over those whose user's ground truth holds it; ids < 0 or >= n_items are skipped"""
    rankings = np.asarray(rankings)
    w = np.asarray(pos_weight).astype(np.int64)
    k = len(w)
    head = rankings[:, :k].astype(np.int64)
    U = head.shape[0]
    valid = (head >= 0) & (head < n_items)
    is_hit = np.zeros_like(valid)
    for u in range(U):
        truth = np.asarray(gt_lists[u], dtype=np.int64)
        if len(truth):
            is_hit[u] = np.isin(head[u], truth)
    is_hit &= valid
    wp = np.broadcast_to(w[None, :], head.shape)
    exp_w = np.zeros(n_items, dtype=np.int64)
    hit_w = np.zeros(n_items, dtype=np.int64)
    np.add.at(exp_w, head[valid], wp[valid])
    np.add.at(hit_w, head[is_hit], wp[is_hit])
    return exp_w, hit_w


def group_sums(group_of, exp_w, hit_w, n_groups):
    out = np.zeros((n_groups, 2), dtype=np.int64)
    for i, g in enumerate(group_of):
        if 0 <= g < n_groups:
            out[g, 0] += exp_w[i]
            out[g, 1] += hit_w[i]
    return out


def gini(x):
    xs = sorted(int(v) for v in x)
    n, total = len(xs), sum(xs)
    if total == 0:
        return float("nan")
    return float(Fraction(sum((2 * r - n - 1) * v for r, v in enumerate(xs, 1)), n * total))


def _share(num, den):
    return float(Fraction(num, den)) if den else float("nan")


def summarize(rec_cnt, exp_w, hit_w, train_counts, group_of, n_groups, users, k):
    rec, ew, hw, train = ([int(v) for v in a] for a in (rec_cnt, exp_w, hit_w, train_counts))
    n = len(rec)
    slots, exp_total, hit_total = sum(rec), sum(ew), sum(hw)
    in_group = lambda vals, g: sum(v for v, gi in zip(vals, group_of) if gi == g)
    return {"users": users, "k": k, "slots": slots, "coverage": sum(1 for v in rec if v > 0) / n,
            "gini": gini(rec), "gini_dcg": gini(ew),
            "arp": _share(sum(r * t for r, t in zip(rec, train)), slots),
            "arp_dcg": _share(sum(e * t for e, t in zip(ew, train)), exp_total),
            "group_exposure": [_share(in_group(ew, g), exp_total) for g in range(n_groups)],
            "group_dcg_hits": [_share(in_group(hw, g), hit_total) for g in range(n_groups)]}


def format_line(rep):
    fl = lambda vals: ", ".join("%.5f" % v for v in vals)
    return ("exposure @%d: users=%d slots=%d coverage=%.5f gini=%.5f gini_dcg=%.5f arp=%.2f arp_dcg=%.2f | train-popularity groups "
            "(<10,<50,<100,<200,<500,>=500): exposure=[%s] dcg_hits=[%s]") % (
        rep["k"], rep["users"], rep["slots"], rep["coverage"], rep["gini"], rep["gini_dcg"], rep["arp"], rep["arp_dcg"],
        fl(rep["group_exposure"]), fl(rep["group_dcg_hits"]))
