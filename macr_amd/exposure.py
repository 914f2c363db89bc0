"""Concentration and position-discounted exposure of an evaluation's top-k lists: the host half of `MACR_EXPOSURE_REPORT=1`.

What a popularity-bias study asks of a recommender besides its accuracy: how much of the catalogue the lists reach
(coverage), how unevenly the slots are spread over the items (Gini), how popular the average recommended item is (ARP) --
and the same with every slot weighted by a browsing model, w[p] = 1 / log2(p + 2) for list position p (the DCG discount):
an unpopular item at the top of a list is exposed more than one at position 20.  The weighted sums over the hits give each
popularity group's share of the DCG mass.

The counting runs on the device (ops.item_counts for the slots, ops.item_exposure for the weighted sums; both through
Evaluator.item_exposure).  The weights are INTEGERS, floor(2^24 / log2(p + 2) + 0.5), so the device sums are exact 64-bit
integers, identical from run to run and for every number of ranks; everything here is bookkeeping on n_items of them, in
Python integers where a product could pass 2^63 and one float64 division per reported figure.  Needs neither torch nor the
native library.
"""
import math
import os

import numpy as np

WEIGHT_ONE = 1 << 24                                  # the weight of position 0
GROUP_LABEL = "<10,<50,<100,<200,<500,>=500"          # popularity.POINTS, as the line names them


def position_weights(k):
    """uint32[k]: w[p] = floor(2^24 / log2(p + 2) + 0.5), the DCG discount of list position p in units of 2^-24"""
    if int(k) < 1:
        raise ValueError("position_weights: k=%r" % (k,))
    return np.array([int(math.floor(WEIGHT_ONE / math.log2(p + 2) + 0.5)) for p in range(int(k))], dtype=np.uint32)


def _ints(x):
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError("exposure: integer counts expected, got %s" % a.dtype)
    return a.astype(np.int64).ravel()


def _ratio(num, den):
    """num / den of two Python integers as a float; nan over a zero total"""
    return float("nan") if den == 0 else num / den


def _dot(a, b):
    """sum a[i] * b[i] as a Python integer (the products of 64-bit sums and train counts may pass 2^63)"""
    return sum(int(x) * int(y) for x, y in zip(a[a != 0].tolist(), b[a != 0].tolist()))


def gini(x):
    """Gini coefficient of non-negative integers over the WHOLE catalogue, zeros included:
    sum_r (2 r - n - 1) x_(r) / (n sum x) over the ascending order x_(1) <= ... <= x_(n); 0 = every item alike,
    (n - 1) / n = one item has everything; nan for an all-zero (or empty) vector.  The numerator is an exact integer."""
    x = np.sort(_ints(x))
    if len(x) and x[0] < 0:
        raise ValueError("gini: negative count")
    n = len(x)
    total = sum(x[x != 0].tolist())
    if total == 0:
        return float("nan")
    coef = 2 * np.arange(1, n + 1, dtype=np.int64) - n - 1
    return _dot(x, coef) / (n * total)


def summarize(rec_cnt, exp_w, hit_w, train_counts, group_of, n_groups, users, k):
    """rec_cnt / exp_w / hit_w int[n_items]: per item the top-k slots that name it, the position-weighted sum over them and
    over the hits among them (Evaluator.item_exposure); train_counts int[n_items] train interactions; group_of int[n_items]
    the popularity group of every item (a value outside [0, n_groups) is in no group).  -> dict
        users, k        as given
        slots           sum of rec_cnt
        coverage        items with rec_cnt > 0, over n_items
        gini, gini_dcg  gini(rec_cnt), gini(exp_w)
        arp             sum rec_cnt train_counts / slots       (average recommendation popularity)
        arp_dcg         sum exp_w train_counts / sum exp_w     (the same, every slot weighted by its position)
        group_exposure  float64[n_groups]: group g's share of sum exp_w
        group_dcg_hits  float64[n_groups]: group g's share of sum hit_w
    A share over a zero total is nan."""
    rec, ew, hw, train, grp = (_ints(a) for a in (rec_cnt, exp_w, hit_w, train_counts, group_of))
    n = len(rec)
    if not (len(ew) == len(hw) == len(train) == len(grp) == n) or n == 0:
        raise ValueError("exposure.summarize: %d / %d / %d / %d / %d items" % (n, len(ew), len(hw), len(train), len(grp)))
    slots = sum(rec[rec != 0].tolist())
    exp_total = sum(ew[ew != 0].tolist())
    hit_total = sum(hw[hw != 0].tolist())
    n_groups = int(n_groups)
    g_exp, g_hit = [0] * n_groups, [0] * n_groups
    for g in range(n_groups):
        mine = grp == g
        g_exp[g] = sum(ew[mine].tolist())
        g_hit[g] = sum(hw[mine].tolist())
    return {"users": int(users), "k": int(k), "slots": int(slots), "coverage": int(np.count_nonzero(rec > 0)) / n,
            "gini": gini(rec), "gini_dcg": gini(ew), "arp": _ratio(_dot(rec, train), slots),
            "arp_dcg": _ratio(_dot(ew, train), exp_total),
            "group_exposure": np.array([_ratio(v, exp_total) for v in g_exp], dtype=np.float64),
            "group_dcg_hits": np.array([_ratio(v, hit_total) for v in g_hit], dtype=np.float64)}


def format_line(rep):
    """the one line an evaluation prints under MACR_EXPOSURE_REPORT=1"""
    return ("exposure @%d: users=%d slots=%d coverage=%.5f gini=%.5f gini_dcg=%.5f arp=%.2f arp_dcg=%.2f | "
            "train-popularity groups (%s): exposure=[%s] dcg_hits=[%s]" % (
                rep["k"], rep["users"], rep["slots"], rep["coverage"], rep["gini"], rep["gini_dcg"], rep["arp"], rep["arp_dcg"],
                GROUP_LABEL, ", ".join("%.5f" % v for v in rep["group_exposure"]),
                ", ".join("%.5f" % v for v in rep["group_dcg_hits"])))


def enabled():
    """MACR_EXPOSURE_REPORT=1 in the environment: every evaluation of the command lines also prints format_line"""
    return os.environ.get("MACR_EXPOSURE_REPORT", "") == "1"
