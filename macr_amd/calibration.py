"""Whether the lists follow each USER's own taste for popularity: the host half of `MACR_CALIBRATION_REPORT`.

MACR's user branch models how far a user follows popularity, and the counterfactual score (y - c) * sigma_i * sigma_u should
move every user's list towards that user's own taste, not merely towards the tail.  The figures that ask this of a
recommender compare, user by user, the popularity mix of the profile (the train list) with the popularity mix of the list:

    js, tv        the Jensen-Shannon divergence (base 2, in [0, 1]) and the total variation distance between the two mixes
                  over the train-popularity groups: Abdollahpouri et al.'s user popularity deviation, Steck's calibration
    gap           the group average popularity: the mean train count of the items of a profile (gap_profile) or a list
                  (gap_list), averaged over a set of users
    lift          (mean gap_list - mean gap_profile) / mean gap_profile of a set of users: Delta-GAP
    taste groups  the users in ascending order of their profile's mean popularity: the first fifth is `niche`, the last
                  fifth `blockbuster`, the rest `diverse`

The counting runs on the device (ops.group_hist through Evaluator.list_calibration): per user the items of each group in
the profile and in the list, the hits among the latter, and the 64-bit sum of the train counts.  Everything there is an
exact integer, identical from run to run and for every number of ranks; everything here is bookkeeping on those integers.
tv is one division of two integers; js is one division of a correctly rounded sum (math.fsum) of integer-weighted
logarithms; every mean is a math.fsum, which does not depend on the order of the users.  Needs neither torch nor the
native library.
"""
import math
import os
from fractions import Fraction

import numpy as np

TASTE = ("niche", "diverse", "blockbuster")
TASTE_LABEL = "niche 20%, diverse 60%, blockbuster 20%"


def _ints(x, what):
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError("calibration: integer %s expected, got %s" % (what, a.dtype))
    return a.astype(np.int64)


def tv(a, b):
    """Total variation distance of two mixes given as integer counts, 1/2 sum |a_g / n - b_g / m| with n = sum a, m = sum b,
    formed as sum |a_g m - b_g n| / (2 n m): an exact Fraction.  Both totals must be positive."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    n, m = sum(a), sum(b)
    if len(a) != len(b) or n <= 0 or m <= 0 or min(a) < 0 or min(b) < 0:
        raise ValueError("calibration.tv: two non-empty mixes over the same groups expected")
    return Fraction(sum(abs(x * m - y * n) for x, y in zip(a, b)), 2 * n * m)


def js(a, b):
    """Jensen-Shannon divergence, base-2 logarithms, of the mixes p = a / n and q = b / m given as integer counts
    (0 log 0 = 0): with s_g = a_g m + b_g n,
        [ sum a_g m log2(2 a_g m / s_g) + sum b_g n log2(2 b_g n / s_g) ] / (2 n m)
    -- integer weights, one correctly rounded sum, one division: exactly 0 for equal mixes, exactly 1 for disjoint ones."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    n, m = sum(a), sum(b)
    if len(a) != len(b) or n <= 0 or m <= 0 or min(a) < 0 or min(b) < 0:
        raise ValueError("calibration.js: two non-empty mixes over the same groups expected")
    terms = []
    for x, y in zip(a, b):
        am, bn = x * m, y * n
        if am:
            terms.append(am * math.log2(2 * am / (am + bn)))
        if bn:
            terms.append(bn * math.log2(2 * bn / (am + bn)))
    return math.fsum(terms) / (2 * n * m)


def taste_groups(keys):
    """keys: one sortable key per user with a profile (the profile's mean popularity), in the order of the evaluated user
    list -> (niche, diverse, blockbuster) lists of positions into `keys`: ascending key, ties by position (stable sort);
    the first floor(n / 5) are niche, the last floor(n / 5) blockbuster, the rest diverse."""
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    cut = len(order) // 5
    return order[:cut], order[cut:len(order) - cut], order[len(order) - cut:]


def _mean(values):
    return float("nan") if not values else math.fsum(values) / len(values)


def _lift(gap_list, gap_profile):
    return float("nan") if not gap_profile == gap_profile or gap_profile == 0 else (gap_list - gap_profile) / gap_profile


def _side(users, prof_cnt, prof_gap, list_cnt, list_hit, list_wsum, gt_sizes):
    """the figures of one ranking over the set `users` (positions of users that are not skipped)"""
    gaps = [int(list_wsum[u, 0]) / int(list_wsum[u, 1]) for u in users]
    with_gt = [u for u in users if gt_sizes[u] > 0]
    gap_profile, gap_list = _mean([prof_gap[u] for u in users]), _mean(gaps)
    return {"users": len(users),
            "js": _mean([js(prof_cnt[u], list_cnt[u]) for u in users]),
            "tv": _mean([float(tv(prof_cnt[u], list_cnt[u])) for u in users]),
            "gap_profile": gap_profile, "gap_list": gap_list, "lift": _lift(gap_list, gap_profile),
            "recall": _mean([int(list_hit[u].sum()) / int(gt_sizes[u]) for u in with_gt])}


def summarize(profile, here, gt_sizes, k, base=None):
    """profile = (cnt int (U, n_groups), wsum int (U, 2)): per user the train items of each group and {sum of train counts,
    train items}; here = (cnt, hit, wsum): the same for the first k slots of the list, with the hits per group
    (Evaluator.list_calibration); gt_sizes int[U]: the size of every user's ground truth; base: optional triple like `here`
    for the factual ranking.  -> dict
        users, skipped, k   users counted, and users left out: an empty profile, a profile or a list with no item in any
                            group -- the per-user figures need both mixes
        js, tv              means over the counted users of js() and tv() between profile and list
        gap_profile, gap_list, lift   mean of the users' profile and list mean popularity (wsum / length), and
                            (gap_list - gap_profile) / gap_profile
        recall              mean of hits_u / |gt_u| over the counted users with a ground truth
        taste               per TASTE name the same dict over the group's counted users; the groups are cut over ALL users
                            with a profile (taste_groups of the exact profile means, Fractions)
        base                with `base`: the same dict (with its own `taste`) for the factual ranking, over the same users
    A mean over no user is nan."""
    p_cnt, p_wsum = _ints(profile[0], "profile counts"), _ints(profile[1], "profile sums")
    sizes = _ints(gt_sizes, "ground-truth sizes").ravel()
    U = p_cnt.shape[0]
    if p_cnt.ndim != 2 or U == 0 or p_wsum.shape != (U, 2) or len(sizes) != U:
        raise ValueError("calibration.summarize: profile of shapes %s / %s for %d ground-truth sizes" % (p_cnt.shape, p_wsum.shape, len(sizes)))
    sides = []
    for name, side in (("here", here), ("base", base)):
        if side is None:
            continue
        cnt, hit, wsum = (_ints(x, "list counts") for x in side)
        if cnt.shape != p_cnt.shape or hit.shape != p_cnt.shape or wsum.shape != (U, 2):
            raise ValueError("calibration.summarize: %s of shapes %s / %s / %s" % (name, cnt.shape, hit.shape, wsum.shape))
        sides.append((name, cnt, hit, wsum))
    with_profile = [u for u in range(U) if p_wsum[u, 1] > 0]
    prof_gap = {u: int(p_wsum[u, 0]) / int(p_wsum[u, 1]) for u in with_profile}
    cuts = taste_groups([Fraction(int(p_wsum[u, 0]), int(p_wsum[u, 1])) for u in with_profile])
    p_total = p_cnt.sum(axis=1)
    # counted: both mixes exist, in EVERY ranking reported (so that here and base speak of the same users)
    counted = [u for u in with_profile if p_total[u] > 0 and all(cnt[u].sum() > 0 for _, cnt, _, _ in sides)]
    keep = set(counted)
    rep = {}
    for name, cnt, hit, wsum in sides:
        part = _side(counted, p_cnt, prof_gap, cnt, hit, wsum, sizes)
        part["taste"] = {t: _side([with_profile[i] for i in cut if with_profile[i] in keep], p_cnt, prof_gap, cnt, hit, wsum, sizes)
                         for t, cut in zip(TASTE, cuts)}
        if name == "here":
            rep.update(part)
        else:
            rep["base"] = part
    rep.update(k=int(k), skipped=U - len(counted))
    return rep


def _f(v):
    return "%.5f" % v


def _taste(part, field, fmt):
    return ", ".join(fmt(part["taste"][t][field]) for t in TASTE)


def format_line(rep):
    """the one line an evaluation prints under MACR_CALIBRATION_REPORT=1; with rep['base'] (value 2) the factual ranking's
    figures follow"""
    line = ("calibration @%d: users=%d skipped=%d js=%.5f tv=%.5f gap_profile=%.2f gap_list=%.2f lift=%.5f | "
            "users by profile popularity (%s): users=[%s] js=[%s] lift=[%s] recall=[%s]" % (
                rep["k"], rep["users"], rep["skipped"], rep["js"], rep["tv"], rep["gap_profile"], rep["gap_list"], rep["lift"],
                TASTE_LABEL, _taste(rep, "users", lambda v: "%d" % v), _taste(rep, "js", _f), _taste(rep, "lift", _f),
                _taste(rep, "recall", _f)))
    if "base" in rep:
        b = rep["base"]
        line += " | normal: js=%.5f tv=%.5f gap_list=%.2f lift=%.5f js=[%s] lift=[%s] recall=[%s]" % (
            b["js"], b["tv"], b["gap_list"], b["lift"], _taste(b, "js", _f), _taste(b, "lift", _f), _taste(b, "recall", _f))
    return line


BASE_IS_THE_LIST = ("MACR_CALIBRATION_REPORT=2: --test normal prints the factual ranking itself, the `normal` part would repeat "
                    "the line: printing the line of value 1")


def enabled():
    """MACR_CALIBRATION_REPORT in the environment: 1 = every evaluation of the command lines also prints format_line, 2 = with
    the factual ranking's figures behind it; anything else (unset, 0, junk) = 0, nothing is launched or printed"""
    return {"1": 1, "2": 2}.get(os.environ.get("MACR_CALIBRATION_REPORT", ""), 0)
