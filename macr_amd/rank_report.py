"""AUC, MRR and rank percentiles of held-out items from their full-catalogue positions: the host half of
`MACR_RANK_REPORT=1` and of `MACR_SHARD_RANK_REPORT=1`.

The positions come from the device (ops.rank_positions / Evaluator.rank_positions, or over item shards
Evaluator.rank_positions_sharded: for every ground-truth pair the number of
the user's candidates ranked before it, -1 for a pair that has no position); everything here is float64 bookkeeping on
n_pairs integers.  The reference carries an `auc_loger` list through both training loops (macr_mf/train.py:386,:459) that
nothing fills; this is what it would have held.

Definitions, per query user with m >= 1 valid pairs at ascending positions p_0 < ... < p_{m-1} among n_cand candidates
(n_items minus the user's train items), Nn = n_cand - m > 0 negatives:
    pair j has p_j - j negatives above it; its percentile is pct_j = (p_j - j) / Nn   (0 = above every negative)
    AUC_q = 1 - mean_j pct_j        RR_q = 1 / (p_0 + 1)
The AUC uses the project's TOTAL order (score descending, ties by ascending item id): a negative whose fp32 score equals
the held-out item's exactly is above or below it by id, not given half credit as the rank-sum AUC with midranks would.
"""
import numpy as np

GROUP_LABEL = "<10,<50,<100,<200,<500,>=500"          # popularity.POINTS, as the line names them


def summarize(pos, gt_ptr, gt_idx, n_cand, group_of=None, n_groups=None):
    """pos int[n_pairs] (-1: no position), gt_ptr int[U+1] / gt_idx int[n_pairs] the ground-truth CSR the positions follow,
    n_cand int[U] candidates per query.  -> dict
        users    queries counted: at least one valid pair and at least one negative
        pairs    their valid pairs
        skipped  every other pair: those at -1 and those of queries without negatives
        auc, mrr the means of AUC_q and RR_q over the counted queries (nan when there is none)
        mpr      the mean of pct over the counted pairs (nan when there is none)
    and with group_of (int[n_items]: the group of every item, 0 .. n_groups-1; n_groups None: max + 1)
        group_pairs  int64[n_groups] counted pairs whose item is in the group
        group_mpr    float64[n_groups] the mean of pct over them (nan for a group without one)"""
    pos = np.asarray(pos, dtype=np.int64)
    ptr = np.asarray(gt_ptr, dtype=np.int64)
    idx = np.asarray(gt_idx, dtype=np.int64)
    n_cand = np.asarray(n_cand, dtype=np.int64)
    U = len(ptr) - 1
    if len(pos) != ptr[-1] or len(idx) != len(pos) or len(n_cand) != U:
        raise ValueError("rank_report.summarize: %d positions, %d items, CSR of %d pairs over %d queries, %d candidate counts"
                         % (len(pos), len(idx), ptr[-1], U, len(n_cand)))
    q_of = np.repeat(np.arange(U, dtype=np.int64), np.diff(ptr))
    valid = pos >= 0
    m = np.bincount(q_of[valid], minlength=U)
    neg = n_cand - m
    counted_q = (m >= 1) & (neg > 0)
    sel = np.flatnonzero(valid & counted_q[q_of])
    # by query, then by position: one stable sort of a combined key (eight times faster than np.lexsort on 2 * 10^5 pairs)
    sel = sel[np.argsort(q_of[sel] * (int(pos.max(initial=0)) + 1) + pos[sel], kind="stable")]
    qs, ps = q_of[sel], pos[sel]
    j = np.arange(len(sel), dtype=np.int64) - np.searchsorted(qs, qs, side="left")      # index within the query
    pct = (ps - j).astype(np.float64) / neg[qs].astype(np.float64)
    users = int(counted_q.sum())
    out = {"users": users, "pairs": int(len(sel)), "skipped": int(len(pos) - len(sel))}
    if users:
        auc_q = 1.0 - np.bincount(qs, weights=pct, minlength=U)[counted_q] / m[counted_q]
        rr_q = 1.0 / (ps[j == 0] + 1.0)
        out.update(auc=float(auc_q.mean()), mrr=float(rr_q.mean()), mpr=float(pct.mean()))
    else:
        out.update(auc=float("nan"), mrr=float("nan"), mpr=float("nan"))
    if group_of is not None:
        group_of = np.asarray(group_of, dtype=np.int64)
        if n_groups is None:
            n_groups = int(group_of.max()) + 1 if len(group_of) else 0
        g = group_of[idx[sel]]
        inside = (g >= 0) & (g < n_groups)                # an item outside every group is in no group's mean
        cnt = np.bincount(g[inside], minlength=n_groups).astype(np.int64)
        tot = np.bincount(g[inside], weights=pct[inside], minlength=n_groups)
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update(group_pairs=cnt, group_mpr=np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan))
    return out


def format_line(rep):
    """the one line an evaluation prints under MACR_RANK_REPORT=1"""
    line = "rank: users=%d pairs=%d skipped=%d auc=%.5f mrr=%.5f mpr=%.5f" % (
        rep["users"], rep["pairs"], rep["skipped"], rep["auc"], rep["mrr"], rep["mpr"])
    if "group_pairs" in rep:
        line += " | train-popularity groups (%s): pairs=[%s] mpr=[%s]" % (
            GROUP_LABEL, ", ".join("%d" % n for n in rep["group_pairs"]), ", ".join("%.5f" % v for v in rep["group_mpr"]))
    return line


def enabled():
    """MACR_RANK_REPORT=1 in the environment: every evaluation of the command lines also prints format_line"""
    import os
    return os.environ.get("MACR_RANK_REPORT", "") == "1"


def shard_enabled():
    """MACR_SHARD_RANK_REPORT=1 in the environment: the same line from Evaluator.rank_report_sharded, which also counts where
    the items are sharded -- several ranks, --row_shard 1 -- and on one rank gives what enabled() gives"""
    import os
    return os.environ.get("MACR_SHARD_RANK_REPORT", "") == "1"


def wanted():
    """either switch: an evaluation prints the line, once"""
    return enabled() or shard_enabled()
