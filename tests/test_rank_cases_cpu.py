"""The cases of tests/rank_cases.py really contain what they exist for (no GPU): the launch geometry restated from
rank_kernels.hip puts every case where it is meant to lie -- at the edges of a column block, in blocks whose tile range crosses
from one column block into the next, in pair lists longer than a chunk of k_rank_finish, a wave of k_rank_cols and a column
block -- and the lists carry the masks the GPU tests speak of.  tests/test_gpu_rank_regimes.py rests on this."""
import os
import re

import numpy as np
import pytest

import rank_cases as rc
from helpers import REPO


def test_geometry_by_hand():
    # one query, one pair, one tile: one unit of work, and a grid of one
    assert rc.geometry([1], 32, 64) == dict(n_cols=1, n_cb=1, T=1, grid=1, W=1, longest=1, straddling=0)
    # 17 pairs are two columns; 33 items two tiles; the bound on the columns is (1 + 1) / 256 + 1 = 1 block
    assert rc.geometry([17, 0], 33, 32) == dict(n_cols=2, n_cb=1, T=2, grid=2, W=2, longest=1, straddling=0)
    # 600 columns in 3 blocks of T = 4 tiles; the host's bound is (600 + 600) / 256 + 1 = 5 blocks, a grid of 20 for W = 12:
    # eight blocks get an empty range, no range holds two tiles
    g = rc.geometry([16] * 600, 128, 128)
    assert (g["n_cb"], g["T"], g["W"], g["grid"], g["longest"], g["straddling"]) == (3, 4, 12, 20, 1, 0)
    # what the existing GPU tests reach: one column block (U = 37), one tile per block (U = 300, K = 20, N = 2000), many tiles
    # in one column block (70001 items)
    assert rc.geometry([rc.PAIR_LENS[q % 5] for q in range(37)], 333, 64)["n_cb"] == 1
    g = rc.geometry([20] * 300, 2000, 64)
    assert (g["n_cb"], g["W"], g["grid"], g["longest"], g["straddling"]) == (3, 189, 189, 1, 0)
    g = rc.geometry([rc.PAIR_LENS[q % 5] for q in range(8)], 70001, 32)
    assert g["n_cb"] == 1 and g["longest"] > 1 and g["straddling"] == 0


@pytest.mark.parametrize("U,n_cb", list(zip(rc.COLS_EDGE_U, (1, 1, 2, 3))))
def test_cols_edge(U, n_cb):
    assert rc.COLS_EDGE_U == (255, 256, 257, 513) and (rc.COLS_EDGE_D, rc.COLS_EDGE_N) == (64, 129)
    g = rc.geometry(rc.cols_edge_lens(U), rc.COLS_EDGE_N, rc.COLS_EDGE_D)
    assert g["n_cols"] == U and g["n_cb"] == n_cb
    # the last column block: full, or with padding columns; at 257 and 513 with one column, i.e. seven waves of padding only
    assert (U % rc.K_RANK_COLS) == {255: 255, 256: 0, 257: 1, 513: 1}[U]
    pairs, mask = rc.cols_edge(U)
    assert [len(r) for r in pairs] == [1] * U
    flat = np.asarray([r[0] for r in pairs])
    assert flat.min() < 0 and flat.max() >= rc.COLS_EDGE_N                       # ids outside the table, on both sides
    assert {0, 3, rc.COLS_EDGE_N - 1} <= set(len(m) for m in mask)
    assert any(set(pairs[q]) & set(mask[q]) for q in range(3, U, 7))


@pytest.mark.parametrize("d,grid,longest", [(128, 256, 7), (64, 512, 4)])
def test_straddle(d, grid, longest):
    assert (rc.STRADDLE_U, rc.STRADDLE_N, rc.STRADDLE_DIMS) == (400, 16533, (128, 64))
    lens = rc.straddle_lens()
    assert len(lens) == 400 and lens[:5] == [0, 1, 5, 17, 40] and lens == lens[:5] * 80
    g = rc.geometry(lens, rc.STRADDLE_N, d)
    assert g == dict(n_cols=560, n_cb=3, T=517, W=1551, grid=grid, longest=longest, straddling=2)
    assert rc.STRADDLE_N % rc.K_RANK_TILE != 0


def test_straddle_sharded():
    assert rc.STRADDLE_SHARDINGS == ((3, "interleaved"), (2, "range"))
    lens = rc.straddle_lens()
    assert rc.shard_sizes(rc.STRADDLE_N, (3, "interleaved")) == [5511] * 3
    g = rc.geometry(lens, 5511, 128)
    assert g == dict(n_cols=560, n_cb=3, T=173, W=519, grid=256, longest=3, straddling=1)
    assert rc.shard_sizes(rc.STRADDLE_N, (2, "range")) == [8267, 8266]
    for n_local in (8267, 8266):
        g = rc.geometry(lens, n_local, 128)
        assert (g["n_cb"], g["T"], g["grid"], g["straddling"]) == (3, 259, 256, 2) and g["longest"] > 1


def test_straddle_lists():
    N = rc.STRADDLE_N
    pairs, mask = rc.straddle()
    assert [len(r) for r in pairs] == rc.straddle_lens()
    assert all(r == sorted(set(r)) for r in pairs)
    flat = np.asarray([g for r in pairs for g in r])
    assert flat.min() < 0 and flat.max() >= N
    assert rc.STRADDLE_MASK_LENS == (0, 3, 70, 700)
    for q in range(rc.STRADDLE_U):
        inside = sorted(set(m for m in mask[q] if 0 <= m < N))
        own = [g for g in pairs[q] if 0 <= g < N]
        extra = 1 if q % 7 == 3 and own else 0
        assert rc.STRADDLE_MASK_LENS[q % 4] <= len(inside) <= rc.STRADDLE_MASK_LENS[q % 4] + extra
        if extra:
            assert own[0] in inside
        assert mask[q] == sorted(mask[q])                          # (k_rank_finish finds a repeated id next to itself)
        if q % 4 == 2:                                             # ids outside [0, N) on both sides, and one id twice
            assert min(mask[q]) < 0 and max(mask[q]) >= N and len(mask[q]) == len(set(mask[q])) + 1
        else:
            assert mask[q] == inside
    # masks on both sides of a chunk of 64, and one of more than ten chunks
    assert any(0 < len(m) < rc.K_FINISH_CHUNK for m in mask) and any(len(m) > 10 * rc.K_FINISH_CHUNK for m in mask)
    assert sum(1 for q in range(3, rc.STRADDLE_U, 7) if set(pairs[q]) & set(mask[q])) >= 40


def test_long_lists():
    assert (rc.LONG_D, rc.LONG_N, rc.LONG_EMPTY) == (32, 4203, 70) and rc.LONG_TAIL == (4203, 64, 65, 128, 129, 513, 1, 1, 1)
    lens = rc.long_lens()
    assert lens == [0] * 70 + [4203, 64, 65, 128, 129, 513, 1, 1, 1]
    # k_rank_cols: a wave is 64 consecutive queries of a block of 256; the first is without pairs altogether
    assert all(l == 0 for l in lens[:64])
    # k_rank_finish: lists of one chunk exactly, a chunk + 1, two chunks, two chunks + 1
    C = rc.K_FINISH_CHUNK
    assert {C, C + 1, 2 * C, 2 * C + 1} <= set(lens)
    # k_rank_cols: a query of more than one wave of columns (32) and of more than a column block (256)
    cols = [(l + rc.K_COL_PAIRS - 1) // rc.K_COL_PAIRS for l in lens]
    assert any(32 < c <= rc.K_RANK_COLS for c in cols) and any(c > rc.K_RANK_COLS for c in cols)
    g = rc.geometry(lens, rc.LONG_N, rc.LONG_D)
    assert g["n_cols"] == sum(cols) == 325 and g["n_cb"] == 2
    assert rc.shard_sizes(rc.LONG_N, rc.LONG_SHARDING) == [1401] * 3
    assert rc.geometry(lens, 1401, rc.LONG_D)["n_cb"] == 2
    pairs, mask = rc.long_lists()
    assert [len(r) for r in pairs] == lens and pairs[rc.LONG_WHOLE] == list(range(rc.LONG_N))
    assert {0, 65, 130} <= set(len(m) for m in mask)
    whole = mask[rc.LONG_WHOLE]
    assert len(whole) == len(set(whole)) == 130 and set(whole) <= set(pairs[rc.LONG_WHOLE])
    assert rc.LONG_NAN_ROW in pairs[rc.LONG_WHOLE]


def test_the_kernel_source_names_this_restatement():
    """the constants and the two grid computations geometry() restates are still what rank_kernels.hip has"""
    src = open(os.path.join(REPO, "macr_amd", "csrc", "rank_kernels.hip")).read()
    assert re.search(r"constexpr int kColPairs = %d;" % rc.K_COL_PAIRS, src)
    assert re.search(r"constexpr int kRankTile = %d;" % rc.K_RANK_TILE, src)
    assert re.search(r"constexpr int kRankWaves = %d;" % (rc.K_RANK_COLS // 32), src) and "kRankCols = 32 * kRankWaves" in src
    assert "p0 += %d)" % rc.K_FINISH_CHUNK in src
    grid_lines = [i for i, l in enumerate(src.splitlines()) if re.match(r"\s*const unsigned grid = ", l)]
    assert len(grid_lines) == 2
    lines = src.splitlines()
    for i in grid_lines:
        assert "std::min<long long>(d <= 64 ? 512 : 256, w_max)" in lines[i]
        assert "tests/rank_cases.py" in lines[i - 1] or "tests/rank_cases.py" in lines[i + 1], lines[i]
    assert src.count("((long long)(std::min<long long>(U, n_pairs) + n_pairs / kColPairs) / kRankCols + 1) * T") == 2
