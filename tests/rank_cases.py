"""Prescribed shapes for the full-catalogue position kernels (macr_amd/csrc/rank_kernels.hip), with a restatement of their launch
geometry.

k_rank_count cuts its work -- (column block, tile) pairs in column-block-major order -- into gridDim.x equal ranges.  Which paths of
it a call runs is decided by totals alone: how many columns of <= 16 pairs the pair lists make (k_rank_cols), how many tiles of 32
items the local table has, and the grid the host picks from an upper bound on both.  geometry() restates that arithmetic from the
host code of macr_rank_positions (macr_rank_shard_counts repeats it with the shard's n_local), so that where a case lies is known
before anything runs: several column blocks, several tiles per block, and blocks whose range crosses from one column block into the
next -- the second trip of the kernel's outer loop.  Only totals are restated: k_rank_cols places a wave's columns with one
atomicAdd, so which query sits in which column is not determined.

tests/test_rank_cases_cpu.py shows without a GPU that every case contains what it exists for; tests/test_gpu_rank_regimes.py runs
them against the oracle.
"""
import numpy as np

import rank_shard_ref

K_COL_PAIRS, K_RANK_TILE, K_RANK_COLS = 16, 32, 256      # kColPairs, kRankTile, kRankCols of rank_kernels.hip
K_FINISH_CHUNK = 64                                      # pairs (and mask entries) k_rank_finish takes per trip
PAIR_LENS = (0, 1, 5, 17, 40)                            # test_gpu_rank_positions.PAIR_LENS


def geometry(pair_lens, n_local, d):
    """What the host and k_rank_count make of a call with these pair lists on a table of n_local rows (integer arithmetic as in
    rank_kernels.hip) -> dict: n_cols, n_cb, T, grid, W, longest (tiles in the longest range of a block), straddling (blocks
    with a multiple of T strictly inside their range: they go through the outer loop more than once)"""
    U, n_pairs = len(pair_lens), int(sum(pair_lens))
    n_cols = sum((l + K_COL_PAIRS - 1) // K_COL_PAIRS for l in pair_lens if l > 0)
    n_cb = (n_cols + K_RANK_COLS - 1) // K_RANK_COLS
    T = (n_local + K_RANK_TILE - 1) // K_RANK_TILE
    w_max = ((min(U, n_pairs) + n_pairs // K_COL_PAIRS) // K_RANK_COLS + 1) * T
    grid = max(1, min(512 if d <= 64 else 256, w_max))
    W = n_cb * T
    longest = straddling = 0
    for b in range(grid):
        lo, hi = W * b // grid, W * (b + 1) // grid
        longest = max(longest, hi - lo)
        straddling += any(lo < k * T < hi for k in range(1, n_cb))
    return dict(n_cols=n_cols, n_cb=n_cb, T=T, grid=grid, W=W, longest=longest, straddling=straddling)


# ---- the cases: (d, n_local, pair lengths per query) ---------------------------------------------------------------------------
COLS_EDGE_U = (255, 256, 257, 513)                       # one column per query: a column block less one, full, plus one, 2 blocks + 1
COLS_EDGE_D, COLS_EDGE_N = 64, 129
STRADDLE_U, STRADDLE_N, STRADDLE_DIMS = 400, 16533, (128, 64)
STRADDLE_SHARDINGS = ((3, "interleaved"), (2, "range"))
STRADDLE_MASK_LENS = (0, 3, 70, 700)
TIE_ROWS = 61                                            # distinct rows of the tie table Q[arange(N) % 61]
LONG_D, LONG_N, LONG_EMPTY = 32, 4203, 70
LONG_TAIL = (4203, 64, 65, 128, 129, 513, 1, 1, 1)
LONG_WHOLE = LONG_EMPTY                                  # the query whose pair list is the whole catalogue
LONG_MASK_LENS = (65, 130, 0)                            # by q % 3: the whole-catalogue query masks 130
LONG_NAN_ROW = 11
LONG_SHARDING = (3, "interleaved")


def cols_edge_lens(U):
    return [1] * U


def straddle_lens():
    return [PAIR_LENS[q % len(PAIR_LENS)] for q in range(STRADDLE_U)]


def long_lens():
    return [0] * LONG_EMPTY + list(LONG_TAIL)


def shard_sizes(n_items, sharding):
    return [s[2] for s in rank_shard_ref.shards(n_items, *sharding)]


def lists(rs, pair_lens, n_local, mask_lens, stray_every=0):
    """Pair lists of the given lengths as test_gpu_rank_positions.lists draws them (distinct ids from [-2, n_local + 2], ascending;
    a list as long as the catalogue IS the catalogue) and masks of mask_lens[q % len(mask_lens)] distinct ids; every seventh
    query masks one of its own pair items; stray_every: every such query's mask also carries ids outside [0, n_local) and one
    id twice."""
    pairs, mask = [], []
    pool = np.arange(-2, n_local + 3)
    for q, n in enumerate(pair_lens):
        pairs.append(list(range(n_local)) if n == n_local else sorted(rs.choice(pool, n, replace=False).tolist()))
        row = set(rs.choice(n_local, mask_lens[q % len(mask_lens)], replace=False).tolist())
        own = [g for g in pairs[q] if 0 <= g < n_local]
        if q % 7 == 3 and own:
            row.add(own[0])
        row = sorted(row)
        if stray_every and q % stray_every == stray_every - 2:
            row = sorted(row + [-3, n_local, n_local + 5] + row[:1])
        mask.append(row)
    return pairs, mask


_cache = {}


def cols_edge(U):
    if ("cols_edge", U) not in _cache:
        rs = np.random.RandomState(4000 + U)
        _cache[("cols_edge", U)] = lists(rs, cols_edge_lens(U), COLS_EDGE_N, (0, 3, COLS_EDGE_N - 1))
    return _cache[("cols_edge", U)]


def straddle():
    if "straddle" not in _cache:
        _cache["straddle"] = lists(np.random.RandomState(4100), straddle_lens(), STRADDLE_N, STRADDLE_MASK_LENS, stray_every=4)
    return _cache["straddle"]


def long_lists():
    if "long_lists" not in _cache:
        _cache["long_lists"] = lists(np.random.RandomState(4200), long_lens(), LONG_N, LONG_MASK_LENS)
    return _cache["long_lists"]
