"""Plain-loop restatement of the list comparison behind MACR_SHIFT_REPORT (macr_list_shift, include/macr_hip.h): two top-k
rankings of the same queries, "base" and "here", compared row by row.  Written from the definition, with Python lists and
sets; imports nothing of macr_amd.

Per query, over the first k slots of each row; a VALID id is 0 <= id < n_items, other slots are skipped:
    n_base, n_here   valid entries of each row
    common           entries of here whose id occurs in base
    first_diff       smallest p < k with base[p] != here[p] (raw slots, -1 included); k if there is none
    footrule         sum over the common ids of |position in base - position in here|
    hits_*           entries of base / here / the common ones whose id is in the query's ground truth
    entered          valid ids of here not in base, ascending, then -1 up to k;  left: the same for base against here
"""
import numpy as np

FIELDS = ("n_base", "n_here", "common", "first_diff", "footrule", "hits_base", "hits_here", "hits_common")


def list_shift(rank_base, rank_here, gt_lists, k, n_items):
    """-> (per_user int32 (U,8), entered int32 (U,k), left int32 (U,k))"""
    U = len(rank_base)
    assert len(rank_here) == U and len(gt_lists) == U and k >= 1
    per_user = np.zeros((U, 8), dtype=np.int32)
    entered = np.full((U, k), -1, dtype=np.int32)
    left = np.full((U, k), -1, dtype=np.int32)
    for u in range(U):
        base = [int(x) for x in rank_base[u][:k]]
        here = [int(x) for x in rank_here[u][:k]]
        assert len(base) == k and len(here) == k
        truth = set(int(x) for x in gt_lists[u])
        at_base = {x: p for p, x in enumerate(base) if 0 <= x < n_items}
        at_here = {x: p for p, x in enumerate(here) if 0 <= x < n_items}
        assert len(at_base) == sum(0 <= x < n_items for x in base), "a row repeats an id"
        assert len(at_here) == sum(0 <= x < n_items for x in here), "a row repeats an id"
        first_diff = k
        for p in range(k):
            if base[p] != here[p]:
                first_diff = p
                break
        kept = [x for x in at_here if x in at_base]
        per_user[u] = (len(at_base), len(at_here), len(kept), first_diff, sum(abs(at_base[x] - at_here[x]) for x in kept),
                       sum(1 for x in at_base if x in truth), sum(1 for x in at_here if x in truth),
                       sum(1 for x in kept if x in truth))
        came = sorted(x for x in at_here if x not in at_base)
        went = sorted(x for x in at_base if x not in at_here)
        entered[u, :len(came)] = came
        left[u, :len(went)] = went
    return per_user, entered, left


def pairs_of(ids):
    """(ptr int32[U+1], idx int32[n]): the non-negative entries of an (U,k) id array, row by row"""
    ptr, idx = [0], []
    for row in ids:
        idx.extend(int(x) for x in row if x >= 0)
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


def full_positions(scores, train_lists, ids):
    """for every non-negative entry of the (U,k) array `ids`, row-major: its 0-based position among the query's candidates
    (the columns outside its train list) by (score descending, id ascending); -1 for a train item"""
    out = []
    for q, row in enumerate(ids):
        train = set(int(x) for x in train_lists[q])
        cand = np.array([i for i in range(scores.shape[1]) if i not in train], dtype=np.int64)
        order = cand[np.lexsort((cand, -scores[q, cand].astype(np.float64)))]
        where = {int(i): p for p, i in enumerate(order)}
        out.extend(where.get(int(x), -1) for x in row if x >= 0)
    return np.asarray(out, dtype=np.int32)
