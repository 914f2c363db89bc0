"""Full-catalogue positions past one column block and 64 pairs: the shapes of tests/rank_cases.py -- column counts at the edges
of a column block, blocks of k_rank_count whose tile range crosses from one column block into the next, pair lists of more
than one chunk of k_rank_finish and more than a column block of k_rank_cols -- through the C ABI on outputs and workspaces
pre-filled with garbage, unsharded and item-sharded, against oracle.score_matrix followed by integer counting (tests/rank_ref.py):
positions EQUAL, scores bit-equal.  Where each case lies in the launch geometry is shown by tests/test_rank_cases_cpu.py."""
import numpy as np
import pytest
import torch

import rank_cases as rc
import test_gpu_rank_positions as base              # raw(), tables(), reference(), check(), _agree()
import test_gpu_rank_shard as shard                 # Sharded, check()

pytestmark = pytest.mark.gpu

dev = base.dev


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- the edges of a column block
@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
@pytest.mark.parametrize("U", rc.COLS_EDGE_U)
def test_cols_edge(ops, U, kind_name):
    """255, 256, 257 and 513 columns: a last column block with one padding column, without any, and with one column only (seven
    of its eight waves hold padding and count nothing)"""
    rs = np.random.RandomState(100 + U)
    P, Q, w, wu = base.tables(rs, U, rc.COLS_EDGE_N, rc.COLS_EDGE_D)
    pairs, mask = rc.cols_edge(U)
    pos, _ = base.check(ops, kind_name, P, None, Q, w, wu, 0.7, kind_name != "SCORE_NORMAL", mask, pairs)
    assert -1 in pos and pos.max() > rc.COLS_EDGE_N // 2


# ----------------------------------------------------------------------------- ranges that cross column blocks
_straddle = {}


def straddle_tables(d):
    """P (a table of 450 rows), a permutation of 400 of them, Q, the branch weights and Q's 61-row tie table; shared and left
    unchanged"""
    if d not in _straddle:
        rs = np.random.RandomState(200 + d)
        P, Q, w, wu = base.tables(rs, rc.STRADDLE_U + 50, rc.STRADDLE_N, d)
        perm = rs.permutation(len(P))[:rc.STRADDLE_U].astype(np.int32)
        _straddle[d] = (P, perm, Q, w, wu, Q[np.arange(rc.STRADDLE_N) % rc.TIE_ROWS].copy())
    return _straddle[d]


@pytest.mark.parametrize("call", ["c_by_value_permuted_users", "c_on_device_plain_users"])
@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_DIRECT_MINUS"])
@pytest.mark.parametrize("d", rc.STRADDLE_DIMS)
def test_straddle(ops, d, kind_name, call):
    """3 column blocks x 517 tiles on a grid of 256 (d 128) / 512 (d 64): every block takes several tiles, two blocks cross a
    column-block boundary and start the outer loop of k_rank_count again"""
    P, perm, Q, w, wu, _ = straddle_tables(d)
    pairs, mask = rc.straddle()
    if call == "c_by_value_permuted_users":         # a permutation into the 450-row table
        _, want = base.check(ops, kind_name, P, perm, Q, w, wu, 0.7, False, mask, pairs)
    else:                                           # the table's first 400 rows as they are
        _, want = base.check(ops, kind_name, P[:rc.STRADDLE_U].copy(), None, Q, w, wu, -1.3, True, mask, pairs)
    assert -1 in want and want.max() > 1 << 13


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
@pytest.mark.parametrize("d", rc.STRADDLE_DIMS)
def test_straddle_ties(ops, d, kind_name):
    """61 distinct item rows: every threshold ties with about 270 items spread over all tiles, so the id rule runs in almost every
    tile, on both sides of every range's edge and of the column-block boundaries"""
    P, perm, _, w, wu, Q61 = straddle_tables(d)
    pairs, mask = rc.straddle()
    _, want = base.check(ops, kind_name, P, perm, Q61, w, wu, 0.4, True, mask, pairs)
    assert -1 in want and want.max() > 1 << 13


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_DIRECT_MINUS"])
def test_straddle_sharded(ops, kind_name):
    """the same tables and lists on 3 interleaved shards (173 tiles each, one straddling block) and 2 range shards (259 tiles,
    two): the oracle's positions from every sharding, and from macr_rank_positions on the whole table"""
    P, perm, Q, w, wu, _ = straddle_tables(128)
    pairs, mask = rc.straddle()
    want = shard.check(ops, kind_name, P, perm, Q, w, wu, 0.7, False, mask, pairs, rc.STRADDLE_SHARDINGS)
    assert -1 in want and want.max() > 1 << 13


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_straddle_sharded_ties(ops, kind_name):
    """the tie path turns the pair's global id into a bound on local rows: with item_stride 3 and with item_lo 8267"""
    P, perm, _, w, wu, Q61 = straddle_tables(128)
    pairs, mask = rc.straddle()
    want = shard.check(ops, kind_name, P, perm, Q61, w, wu, 0.4, True, mask, pairs, rc.STRADDLE_SHARDINGS)
    assert -1 in want and want.max() > 1 << 13


# ----------------------------------------------------------------------------- long pair lists
@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI"])
def test_long_lists(ops, kind_name):
    """70 queries without pairs (a whole wave of k_rank_cols), then lists of 4203 (the catalogue: 263 columns, more than a column
    block), 64, 65, 128, 129 (one chunk of k_rank_finish, two, and one pair more) and 513 (33 columns, more than a wave);
    masks of 0, 65 and 130 ids; one NaN item row"""
    rs = np.random.RandomState(300)
    U, N = len(rc.long_lens()), rc.LONG_N
    P, Q, w, wu = base.tables(rs, U, N, rc.LONG_D)
    Q[rc.LONG_NAN_ROW] = np.nan
    pairs, mask = rc.long_lists()
    pos, want = base.check(ops, kind_name, P, None, Q, w, wu, 0.3, False, mask, pairs)
    # the whole-catalogue query: its items that are neither masked nor NaN take every position once
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in pairs])])
    mine = pos[ptr[rc.LONG_WHOLE]:ptr[rc.LONG_WHOLE + 1]]
    count = N - len(set(mask[rc.LONG_WHOLE]) | {rc.LONG_NAN_ROW})
    assert len(mine) == N and count == N - 131
    assert np.array_equal(np.sort(mine[mine >= 0]), np.arange(count))
    assert np.all(mine[sorted(set(mask[rc.LONG_WHOLE]) | {rc.LONG_NAN_ROW})] == -1)
    # item-sharded: the same positions from three interleaved shards
    got = shard.check(ops, kind_name, P, None, Q, w, wu, 0.3, False, mask, pairs, [rc.LONG_SHARDING], whole=False)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- the evaluator
@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_evaluator_positions_of_100_pairs_per_query_agree_with_rank(ops, kind_name):
    """the model of test_evaluator_positions_agree_with_rank_mf with K = 100: two chunks of k_rank_finish behind
    Evaluator.rank_positions, against the wide ranking"""
    rs = np.random.RandomState(21)
    U, n_users, N = 300, 320, 2000
    model = base._mf_model(rs, n_users, N)
    model.update_c(None, 0.7)
    kind = getattr(ops, kind_name)
    uid_np = rs.permutation(n_users)[:U].astype(np.int32)
    uid = dev(uid_np)
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(U)]
    base._agree(ops, (mask, N, uid_np), (kind, model.user_embedding, uid, model.item_embedding),
                dict(w=model.w, wu=model.w_user, c=model.rubi_c), lambda u, i: model.predict(kind, u, i), K=100)
