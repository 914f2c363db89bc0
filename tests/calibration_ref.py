"""Plain-loop restatement of the per-row group histogram behind MACR_CALIBRATION_REPORT (macr_group_hist, include/macr_hip.h) and
of the report's host half (macr_amd/calibration.py::summarize).  Written from the definitions, with Python integers,
fractions.Fraction for tv and math.log2 for js; imports nothing of macr_amd.

Kernel, per row u (ranking form: the first k slots of a row; CSR form: a list of any length); a VALID id is 0 <= id < n_items:
    cnt[u, g]   valid entries with group_of[id] == g (a group outside [0, n_groups) is in no column)
    hit[u, g]   those of them whose id is in the row's ground truth
    wsum[u]     (sum of item_weight[id] over the valid entries -- 0 without weights --, number of valid entries)
"""
import math
from fractions import Fraction

import numpy as np

TASTE = ("niche", "diverse", "blockbuster")


def group_hist(rows, group_of, n_groups, n_items, gt_lists=None, item_weight=None, k=None):
    """rows: a list of id lists (CSR form) or a 2-D array read over its first k columns (k None: all)
    -> (cnt int32 (U, n_groups), hit int32 (U, n_groups) or None, wsum int64 (U, 2))"""
    U = len(rows)
    cnt = np.zeros((U, n_groups), dtype=np.int32)
    hit = np.zeros((U, n_groups), dtype=np.int32) if gt_lists is not None else None
    wsum = np.zeros((U, 2), dtype=np.int64)
    for u in range(U):
        row = [int(x) for x in (rows[u] if k is None else rows[u][:k])]
        truth = set(int(x) for x in gt_lists[u]) if gt_lists is not None else set()
        total, valid = 0, 0
        for i in row:
            if not 0 <= i < n_items:
                continue
            valid += 1
            if item_weight is not None:
                total += int(item_weight[i])
            g = int(group_of[i])
            if 0 <= g < n_groups:
                cnt[u, g] += 1
                if hit is not None and i in truth:
                    hit[u, g] += 1
        assert -2 ** 63 <= total < 2 ** 63
        wsum[u] = (total, valid)
    return cnt, hit, wsum


def tv(a, b):
    """1/2 sum |a_g / n - b_g / m| as an exact Fraction"""
    n, m = sum(int(x) for x in a), sum(int(x) for x in b)
    return sum((abs(Fraction(int(x), n) - Fraction(int(y), m)) for x, y in zip(a, b)), Fraction(0)) / 2


def js(a, b):
    """Jensen-Shannon divergence with base-2 logarithms of p = a / n, q = b / m; 0 log 0 = 0"""
    n, m = sum(int(x) for x in a), sum(int(x) for x in b)
    total = 0.0
    for x, y in zip(a, b):
        p, q = int(x) / n, int(y) / m
        mid = (p + q) / 2
        if p:
            total += 0.5 * p * math.log2(p / mid)
        if q:
            total += 0.5 * q * math.log2(q / mid)
    return total


def taste_cuts(gaps):
    """gaps: {user: exact mean popularity of its profile} in the order of the evaluated user list -> three user lists"""
    users = list(gaps)
    order = sorted(users, key=lambda u: (gaps[u], users.index(u)))
    cut = len(order) // 5
    return order[:cut], order[cut:len(order) - cut], order[len(order) - cut:]


def _mean(vals):
    vals = list(vals)
    return float("nan") if not vals else float(sum(Fraction(v) for v in vals) / len(vals))


def _side(users, p_cnt, p_wsum, cnt, hit, wsum, gt_sizes):
    gp = _mean(Fraction(int(p_wsum[u][0]), int(p_wsum[u][1])) for u in users)
    gl = _mean(Fraction(int(wsum[u][0]), int(wsum[u][1])) for u in users)
    return {"users": len(users), "js": _mean(js(p_cnt[u], cnt[u]) for u in users), "tv": _mean(tv(p_cnt[u], cnt[u]) for u in users),
            "gap_profile": gp, "gap_list": gl, "lift": float("nan") if not users or gp == 0 else (gl - gp) / gp,
            "recall": _mean(Fraction(int(sum(hit[u])), int(gt_sizes[u])) for u in users if gt_sizes[u] > 0)}


def summarize(profile, here, gt_sizes, k, base=None):
    """the report dict of macr_amd/calibration.py::summarize, by plain loops and exact rational means"""
    p_cnt, p_wsum = profile
    U = len(p_cnt)
    sides = [s for s in (here, base) if s is not None]
    with_profile = [u for u in range(U) if p_wsum[u][1] > 0]
    counted = [u for u in with_profile if sum(p_cnt[u]) > 0 and all(sum(s[0][u]) > 0 for s in sides)]
    cuts = taste_cuts({u: Fraction(int(p_wsum[u][0]), int(p_wsum[u][1])) for u in with_profile})
    out = []
    for cnt, hit, wsum in sides:
        part = _side(counted, p_cnt, p_wsum, cnt, hit, wsum, gt_sizes)
        part["taste"] = {t: _side([u for u in cut if u in counted], p_cnt, p_wsum, cnt, hit, wsum, gt_sizes)
                         for t, cut in zip(TASTE, cuts)}
        out.append(part)
    rep = dict(out[0], k=int(k), skipped=U - len(counted))
    if base is not None:
        rep["base"] = out[1]
    return rep
