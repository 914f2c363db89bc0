"""NumPy restatement of the item-sharded position count (macr_rank_shard_keys / _counts / _combine), shared by
tests/test_rank_shard_cpu.py and tests/test_gpu_rank_shard.py, on tests/rank_ref.py's key: a shard (item_lo, item_stride,
n_local) holds the global items item_lo + l * item_stride, pair and mask ids are global, a shard's outputs are int64 arrays
that are summed over the shards (with wrap-around, as an int64 all-reduce sums)."""
import numpy as np

import rank_ref

MASKED = 1 << 40                 # MACR_RANK_SHARD_MASKED
NO_OWNER, NO_KEY = np.uint64(0), np.uint64(0xffffffffffffffff)


def shards(n_items, world, layout):
    """[(item_lo, item_stride, n_local)] of the `world` shards: "interleaved" (sharded_train.Owned: item g on rank g % world)
    or "range" (sharding.item_shard_range); n_local is 0 where there are fewer items than ranks"""
    if layout == "interleaved":
        return [(r, world, len(range(r, n_items, world))) for r in range(world)]
    base, rem = divmod(n_items, world)
    return [(r * base + min(r, rem), 1, base + (1 if r < rem else 0)) for r in range(world)]


def owned(shard):
    lo, stride, n = shard
    return lo + stride * np.arange(n, dtype=np.int64)


def global_keys(scores_row, ids):
    """rank_ref.keys of the given columns of a score row with their GLOBAL ids in the low word; all-ones for a NaN"""
    k = rank_ref.keys(scores_row)[ids]                  # (rank_ref.keys numbers the columns 0 .. N-1: the global ids)
    k[np.isnan(scores_row[ids])] = NO_KEY
    return k


def shard_keys(scores, shard, pair_lists):
    """uint64[n_pairs]: the key of a pair whose item the shard owns, all-ones where that score is NaN, 0 elsewhere"""
    mine = set(owned(shard).tolist())
    out = []
    for q, row in enumerate(pair_lists):
        for g in row:
            out.append(global_keys(scores[q], np.asarray([g]))[0] if g in mine else NO_OWNER)
    return np.asarray(out, dtype=np.uint64)


def shard_counts(scores, shard, mask_lists, pair_lists, keys):
    """int64[n_pairs]: the shard's items before the key, minus its own mask items of the query before the key, plus MASKED
    where it owns the pair's item and the query masks it; 0 for a key of 0 or all-ones"""
    ids = owned(shard)
    mine = set(ids.tolist())
    out, p = [], 0
    for q, row in enumerate(pair_lists):
        k_all = global_keys(scores[q], ids) if len(ids) else np.zeros(0, dtype=np.uint64)
        k_all = np.where(k_all == NO_KEY, NO_OWNER, k_all)            # a NaN candidate is before nothing
        m = np.asarray(sorted({i for i in mask_lists[q] if i in mine}), dtype=np.int64)
        k_mask = global_keys(scores[q], m) if len(m) else np.zeros(0, dtype=np.uint64)
        k_mask = np.where(k_mask == NO_KEY, NO_OWNER, k_mask)
        for g in row:
            k = keys[p]
            p += 1
            if k == NO_OWNER or k == NO_KEY:
                out.append(0)
                continue
            cnt = int((k_all > k).sum()) - int((k_mask > k).sum())
            out.append(cnt + (MASKED if g in mine and g in set(mask_lists[q]) else 0))
    return np.asarray(out, dtype=np.int64)


def sum_int64(arrays):
    """what an int64 all-reduce SUM leaves: element-wise, wrapping"""
    total = np.zeros_like(np.asarray(arrays[0]).view(np.int64))
    for a in arrays:
        total = total + np.asarray(a).view(np.int64)
    return total


def combine(keys, summed):
    """int32[n_pairs]: -1 where the key is 0 or all-ones or the flag bit is set, else the low 31 bits of the sum"""
    keys = np.asarray(keys).view(np.uint64)
    summed = np.asarray(summed, dtype=np.int64)
    bad = (keys == NO_OWNER) | (keys == NO_KEY) | ((summed & MASKED) != 0)
    return np.where(bad, -1, summed & 0x7fffffff).astype(np.int32)


def positions(scores, world, layout, mask_lists, pair_lists):
    """the three calls on every shard, summed as the collectives sum: int32[n_pairs]"""
    parts = shards(scores.shape[1], world, layout)
    keys = sum_int64([shard_keys(scores, s, pair_lists) for s in parts]).view(np.uint64)
    counts = sum_int64([shard_counts(scores, s, mask_lists, pair_lists, keys) for s in parts])
    return combine(keys, counts)
