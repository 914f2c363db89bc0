"""NumPy restatement of the per-item accuracy diagnostic (the reference's item_acc_list, macr_mf/train.py:261-277 and
macr_lightgcn/utility/batch_test.py:94-115, plus the popularity-group table): scores, train lists and test lists in;
top-k outside train by (score descending, id ascending), counts, dictionary and group table out.  Written from the
reference's loops, independent of macr_amd/popularity.py; tests/golden/G15_item_acc.json pins it to the reference."""
import numpy as np


def rank_outside_train(scores, train_lists, K):
    """(U,K) int32: each row's K best columns outside its train list, score descending, ties by ascending id; -1 where
    the row has fewer candidates"""
    U, N = scores.shape
    out = np.full((U, K), -1, dtype=np.int32)
    for q in range(U):
        cand = np.setdiff1d(np.arange(N), np.asarray(train_lists[q], dtype=np.int64))
        order = cand[np.lexsort((cand, -scores[q, cand].astype(np.float64)))][:K]
        out[q, :len(order)] = order
    return out


def item_counts(rankings, gt_lists, k, n_items):
    """(rec_cnt, hit_cnt) int64[n_items] over the first k ids of every row (ids < 0 skipped)"""
    rec = np.zeros(n_items, dtype=np.int64)
    hit = np.zeros(n_items, dtype=np.int64)
    for q, row in enumerate(rankings):
        truth = set(int(x) for x in gt_lists[q])
        for i in row[:k]:
            if i < 0:
                continue
            rec[i] += 1
            if int(i) in truth:
                hit[i] += 1
    return rec, hit


def group_sums(group_of, rec, hit, n_groups):
    out = np.zeros((n_groups, 2), dtype=np.int64)
    for i, g in enumerate(group_of):
        if 0 <= g < n_groups:
            out[g, 0] += rec[i]
            out[g, 1] += hit[i]
    return out


def n_test_of(test_lists, n_items):
    """test interactions per item, every occurrence counted (len(test_item_list[i]))"""
    n = np.zeros(n_items, dtype=np.int64)
    for row in test_lists:
        for i in row:
            n[i] += 1
    return n


def acc_dict(hit, n_test):
    """the reference's dictionary: int 0, then `+= 1/len(...)` once per hit"""
    d = {}
    for i in range(len(hit)):
        d[i] = 0
    for i in range(len(hit)):
        for _ in range(int(hit[i])):
            d[i] += 1 / int(n_test[i])
    return d


def groups_of(train_counts, points=(10, 50, 100, 200, 500)):
    """plot_pics' walk (macr_mf/load_data.py:438-443) per item instead of over the sorted counts"""
    out = []
    for c in train_counts:
        p = 0
        while p != len(points) and points[p] < c:
            p += 1
        out.append(p)
    return np.asarray(out, dtype=np.int32)


def group_table(group_of, rec, hit, n_test, n_groups=6):
    n_items, slots = len(group_of), int(np.sum(rec))
    rows = []
    for g in range(n_groups):
        ids = [i for i in range(n_items) if group_of[i] == g]
        test = int(sum(n_test[i] for i in ids))
        hits = int(sum(hit[i] for i in ids))
        accs = [hit[i] / n_test[i] for i in ids if n_test[i] > 0]
        rows.append({"items": len(ids), "catalogue_share": len(ids) / n_items,
                     "slot_share": int(sum(rec[i] for i in ids)) / slots if slots else 0.0, "hits": hits, "test": test,
                     "recall": hits / test if test else 0.0, "mean_item_acc": float(np.mean(accs)) if accs else 0.0})
    return rows


def item_accuracy(scores, train_lists, test_lists, k, all_test_lists=None):
    """scores (U,N) of the evaluated users, their train and test lists -> (rec, hit, n_test, dictionary).
    all_test_lists: the lists the denominators count (default: the evaluated users')"""
    n_items = scores.shape[1]
    rec, hit = item_counts(rank_outside_train(scores, train_lists, k), test_lists, k, n_items)
    n_test = n_test_of(test_lists if all_test_lists is None else all_test_lists, n_items)
    return rec, hit, n_test, acc_dict(hit, n_test)
