"""What the inference-time correction changed, user by user: the host half of `MACR_SHIFT_REPORT`.

MACR ranks by (y - c) * sigma_i * sigma_u in place of y.  The metrics of `--test normal` and `--test rubi` are two aggregate
lines; the paired questions -- how much of a user's list was replaced and how high up, which popularity groups the replaced
slots went to and came from, how many hits the correction gained and lost ON THE SAME USERS, how deep in the uncorrected
ranking the promoted items stood -- need both rankings of every user side by side.

The comparing runs on the device (ops.list_shift for the lists, ops.item_counts for the per-item and per-group sums,
ops.rank_positions for the depths; all through Evaluator.list_shift / shift_depth).  Everything there is an exact integer,
identical from run to run and for every number of ranks; everything here is bookkeeping on those integers, totals as Python
integers (they may pass 2^31) and one float64 division per reported figure.  Needs neither torch nor the native library.
"""
import os
from fractions import Fraction

import numpy as np

GROUP_LABEL = "<10,<50,<100,<200,<500,>=500"          # popularity.POINTS, as the line names them
FIELDS = ("n_base", "n_here", "common", "first_diff", "footrule", "hits_base", "hits_here", "hits_common")


def _ints(x, what):
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError("shift_report: integer %s expected, got %s" % (what, a.dtype))
    return a.astype(np.int64)


def _total(a):
    """the sum of an integer array as a Python integer"""
    return sum(a[a != 0].tolist())


def _ratio(num, den):
    """num / den of two Python integers as a float; nan over a zero total"""
    return float("nan") if den == 0 else num / den


def sign_test(better, worse):
    """The exact two-sided sign test of `better` users against `worse` (ties dropped): with n = better + worse,
    min(1, 2 * sum_{i <= min(better, worse)} C(n, i) / 2^n) as a Fraction; 1 at n = 0.  Python integers throughout
    (C(n, i + 1) = C(n, i) (n - i) / (i + 1)), so the value is exact for any n."""
    better, worse = int(better), int(worse)
    if better < 0 or worse < 0:
        raise ValueError("sign_test: better=%d worse=%d" % (better, worse))
    n, m = better + worse, min(better, worse)
    term, tail = 1, 0
    for i in range(m + 1):
        tail += term
        term = term * (n - i) // (i + 1)
    return min(Fraction(1), Fraction(2 * tail, 1 << n))


def _nearest_rank(sorted_vals, num, den):
    """the num/den quantile of ascending integers by the nearest-rank rule: the element at ceil(num n / den) - 1"""
    n = len(sorted_vals)
    return None if n == 0 else int(sorted_vals[max((num * n + den - 1) // den - 1, 0)])


def summarize_depth(pos_entered, pos_left):
    """pos_entered / pos_left int[...]: the 0-based full-ranking positions of Evaluator.shift_depth (-1: no position) ->
    {'entered': (median, 90th percentile, max), 'left': (...), 'skipped'}: nearest-rank quantiles of the positions >= 0 --
    integers that occur in the data -- None where there is none; skipped counts the -1 of both."""
    out, skipped = {}, 0
    for name, pos in (("entered", pos_entered), ("left", pos_left)):
        p = _ints(pos, "positions").ravel()
        v = np.sort(p[p >= 0])
        skipped += int(len(p) - len(v))
        out[name] = (_nearest_rank(v, 1, 2), _nearest_rank(v, 9, 10), None if len(v) == 0 else int(v[-1]))
    out["skipped"] = skipped
    return out


def summarize(per_user, entered_rec, entered_hit, left_rec, left_hit, group_of, n_groups, k, depth=None, base="normal"):
    """per_user int (U, 8): FIELDS per query (ops.list_shift); entered_rec / entered_hit int[n_items]: how often each item
    entered a list and how often as a gained hit, left_rec / left_hit the same for the items that left and the lost hits
    (ops.item_counts of the entered / left lists); group_of int[n_items] the popularity group of every item (a value
    outside [0, n_groups) is in no group); depth: optional (pos_entered, pos_left) of Evaluator.shift_depth.  -> dict
        users, k, base      as given
        identical           users with first_diff == k: the same list, slot for slot
        overlap             sum common / sum n_here
        first_diff          its mean over the users
        footrule            sum footrule / sum common: the mean displacement of a kept item
        hits_base, hits_here, kept, gained, lost   sums of hits_base, hits_here, hits_common, hits_here - hits_common,
                            hits_base - hits_common
        better, worse       users with hits_here above / below hits_base
        sign_p              sign_test(better, worse) as a float
        group_entered, group_left   float64[n_groups]: group g's share of the entered / left slots
        group_gained, group_lost    int64[n_groups]: its gained / lost hits
        depth               summarize_depth(*depth), when given
    A ratio over a zero total is nan."""
    pu = _ints(per_user, "per-user rows")
    if pu.ndim != 2 or pu.shape[1] != len(FIELDS) or pu.shape[0] == 0:
        raise ValueError("shift_report.summarize: per_user of shape %s, (U >= 1, %d) expected" % (pu.shape, len(FIELDS)))
    k = int(k)
    col = {name: pu[:, j] for j, name in enumerate(FIELDS)}
    er, eh, lr, lh, grp = (_ints(a, "counts").ravel() for a in (entered_rec, entered_hit, left_rec, left_hit, group_of))
    n = len(grp)
    if not (len(er) == len(eh) == len(lr) == len(lh) == n) or n == 0:
        raise ValueError("shift_report.summarize: %d / %d / %d / %d / %d items" % (len(er), len(eh), len(lr), len(lh), n))
    tot = {name: _total(col[name]) for name in FIELDS}
    gained, lost = tot["hits_here"] - tot["hits_common"], tot["hits_base"] - tot["hits_common"]
    better = int(np.count_nonzero(col["hits_here"] > col["hits_base"]))
    worse = int(np.count_nonzero(col["hits_here"] < col["hits_base"]))
    n_groups = int(n_groups)
    sums = [[_total(a[grp == g]) for g in range(n_groups)] for a in (er, lr, eh, lh)]
    ent_total, left_total = _total(er), _total(lr)
    rep = {"users": int(pu.shape[0]), "k": k, "base": str(base),
           "identical": int(np.count_nonzero(col["first_diff"] == k)),
           "overlap": _ratio(tot["common"], tot["n_here"]),
           "first_diff": _ratio(tot["first_diff"], int(pu.shape[0])),
           "footrule": _ratio(tot["footrule"], tot["common"]),
           "hits_base": tot["hits_base"], "hits_here": tot["hits_here"], "kept": tot["hits_common"], "gained": gained, "lost": lost,
           "better": better, "worse": worse, "sign_p": float(sign_test(better, worse)),
           "group_entered": np.array([_ratio(v, ent_total) for v in sums[0]], dtype=np.float64),
           "group_left": np.array([_ratio(v, left_total) for v in sums[1]], dtype=np.float64),
           "group_gained": np.array(sums[2], dtype=np.int64), "group_lost": np.array(sums[3], dtype=np.int64)}
    if depth is not None:
        rep["depth"] = summarize_depth(*depth)
    return rep


def _pos(v):
    return "nan" if v is None else "%d" % v


def format_line(rep):
    """the one line an evaluation prints under MACR_SHIFT_REPORT=1; with rep['depth'] (value 2) the depth part follows"""
    line = ("shift @%d vs %s: users=%d identical=%d overlap=%.5f first_diff=%.3f footrule=%.3f | "
            "hits base=%d here=%d kept=%d gained=%d lost=%d users better=%d worse=%d sign_p=%.4g | "
            "train-popularity groups (%s): entered=[%s] left=[%s] gained=[%s] lost=[%s]" % (
                rep["k"], rep["base"], rep["users"], rep["identical"], rep["overlap"], rep["first_diff"], rep["footrule"],
                rep["hits_base"], rep["hits_here"], rep["kept"], rep["gained"], rep["lost"], rep["better"], rep["worse"], rep["sign_p"],
                GROUP_LABEL, ", ".join("%.5f" % v for v in rep["group_entered"]), ", ".join("%.5f" % v for v in rep["group_left"]),
                ", ".join("%d" % v for v in rep["group_gained"]), ", ".join("%d" % v for v in rep["group_lost"])))
    if "depth" in rep:
        d = rep["depth"]
        line += " | depth: entered med=%s p90=%s max=%s left med=%s p90=%s max=%s (skipped=%d)" % (
            tuple(_pos(v) for v in d["entered"]) + tuple(_pos(v) for v in d["left"]) + (d["skipped"],))
    return line


NOTHING_TO_COMPARE = ("MACR_SHIFT_REPORT: --test normal prints the factual ranking itself, there is nothing to compare it with: "
                      "no shift line")


def enabled():
    """MACR_SHIFT_REPORT in the environment: 1 = every evaluation of the command lines whose score kind is not `normal` also
    prints format_line, 2 = with the depth part; anything else (unset, 0, junk) = 0, nothing is launched or printed"""
    return {"1": 1, "2": 2}.get(os.environ.get("MACR_SHIFT_REPORT", ""), 0)


def refusal(sharded):
    """the message a command line exits with when MACR_SHIFT_REPORT=2 meets an item-sharded evaluation (`sharded`: how the
    run is sharded, in words)"""
    return ("MACR_SHIFT_REPORT=2 adds full-catalogue positions, counted over a whole, replicated item table: it has no %s form; "
            "set MACR_SHIFT_REPORT=1 for the line without the depth part, or evaluate on one rank" % sharded)
