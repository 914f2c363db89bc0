"""Per-item accuracy and popularity-group diagnostics: the host half of `--out 1`.

The reference builds an `item_acc_list` in both test() functions (macr_mf/train.py:261-277 with k = 5,
macr_lightgcn/utility/batch_test.py:94-115 with k = 20, written to Lightgcn_macr.txt) and its MF loader cuts the items
into six popularity groups (plot_pics, macr_mf/load_data.py:424-466).  The counting runs on the device
(ops.item_counts / Evaluator.item_accuracy); everything here is bookkeeping on n_items numbers.
"""
import numpy as np

POINTS = (10, 50, 100, 200, 500)          # plot_pics' cut points, in train interactions (load_data.py:430)


def item_groups(train_counts, points=POINTS):
    """int32[n_items]: the popularity group of every item = the number of cut points strictly below its train count
    (plot_pics' `while points[p] < score: p += 1`, load_data.py:438-443); an item without a train interaction is in
    group 0 (the reference's loop never sees it: it walks train_item_list)."""
    counts = np.asarray(train_counts, dtype=np.int64)
    return np.searchsorted(np.asarray(points, dtype=np.int64), counts, side="left").astype(np.int32)


def train_counts(train_item_list, n_items):
    """int64[n_items] train interactions per item from a {item: [users...]} mapping (MFData.train_item_list)"""
    counts = np.zeros(n_items, dtype=np.int64)
    for item, users in train_item_list.items():
        counts[item] = len(users)
    return counts


def item_acc_dict(hit_cnt, n_test):
    """The reference's item_acc_list: {item: accuracy} over range(n_items), built with the reference's own accumulation --
    int 0 for an item no hit touched, else hit_cnt[i] repeated float64 additions of 1 / n_test[i] (`+= 1/len(...)`,
    train.py:277, batch_test.py:113) -- so that str() of it is the content of the reference's file."""
    hit_cnt = np.asarray(hit_cnt)
    n_test = np.asarray(n_test)
    acc = {i: 0 for i in range(len(hit_cnt))}
    for i in np.flatnonzero(hit_cnt):
        if n_test[i] <= 0:
            raise ValueError("item %d has %d hits but no test interaction" % (i, hit_cnt[i]))
        step, v = 1 / int(n_test[i]), 0
        for _ in range(int(hit_cnt[i])):
            v += step
        acc[int(i)] = v
    return acc


def group_report(group_of, rec_cnt, hit_cnt, n_test, n_groups=len(POINTS) + 1, group_sums=None):
    """Per popularity group, a dict of
        items            items of the group
        catalogue_share  items / n_items                 (plot_pics' `rate`, over the whole catalogue)
        slot_share       share of all filled top-k slots that name an item of the group
        hits             top-k slots that name a test item of their user
        test             test interactions of the group's items (every occurrence in the file)
        recall           hits / test (0.0 for a group without test interactions)
        mean_item_acc    mean of hit_cnt / n_test over the group's items that have test interactions (0.0 if none)
    group_sums: the (n_groups, 2) {rec, hit} sums ops.item_counts computed on the device; None: summed here."""
    group_of = np.asarray(group_of)
    rec_cnt, hit_cnt, n_test = (np.asarray(a, dtype=np.int64) for a in (rec_cnt, hit_cnt, n_test))
    n_items = len(group_of)
    if group_sums is None:
        group_sums = np.stack([np.bincount(group_of, weights=rec_cnt, minlength=n_groups),
                               np.bincount(group_of, weights=hit_cnt, minlength=n_groups)], axis=1)
    group_sums = np.asarray(group_sums, dtype=np.int64)
    slots = int(group_sums[:, 0].sum())
    tested = n_test > 0
    acc = np.zeros(n_items, dtype=np.float64)
    acc[tested] = hit_cnt[tested] / n_test[tested]
    rows = []
    for g in range(n_groups):
        mine = group_of == g
        items, test = int(mine.sum()), int(n_test[mine].sum())
        rec, hits = int(group_sums[g, 0]), int(group_sums[g, 1])
        with_test = mine & tested
        rows.append({"items": items, "catalogue_share": items / n_items, "slot_share": rec / slots if slots else 0.0,
                     "hits": hits, "test": test, "recall": hits / test if test else 0.0,
                     "mean_item_acc": float(acc[with_test].mean()) if with_test.any() else 0.0})
    return rows


def format_report(rows, k):
    """the one line an evaluation prints under --out 1"""
    return "item groups @%d: catalogue=[%s] slots=[%s] recall=[%s]" % (
        k, ", ".join("%.5f" % r["catalogue_share"] for r in rows), ", ".join("%.5f" % r["slot_share"] for r in rows),
        ", ".join("%.5f" % r["recall"] for r in rows))


def emit(rec_cnt, hit_cnt, group_sums, n_test, group_of, k, path):
    """What the main rank does with an evaluation's counts under --out 1: str(item_acc_dict) into `path` (overwritten at
    every evaluation, as batch_test.py:114-115 does) and the group line on stdout.  -> (dictionary, group rows)"""
    to_np = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    rec_cnt, hit_cnt, group_sums = to_np(rec_cnt), to_np(hit_cnt), to_np(group_sums)
    acc = item_acc_dict(hit_cnt, n_test)
    with open(path, "w+") as f:
        f.write(str(acc))
    rows = group_report(group_of, rec_cnt, hit_cnt, n_test, n_groups=len(group_sums), group_sums=group_sums)
    print(format_report(rows, k))
    return acc, rows
