"""Evaluator.list_shift / shift_depth / rank_positions(pairs=...) (MACR_SHIFT_REPORT) on a small random MF model against a host
full sort of macr_score_matrix's output under the project's tie rule (score descending, ties by ascending id, train items
excluded) and the plain-loop restatement (tests/shift_ref.py).  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

import item_acc_ref
import shift_ref as R

pytestmark = pytest.mark.gpu

K = 20
C = 0.7


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", params=[32, 64])
def model(ops, request):
    """300 query users of 320 x 500 items, item rows with a popularity direction the item branch picks up, hand-set w and
    w_user; train lists of 0 .. 30 items, ground truth of 0 .. 6 items plus, for every seventh user, one item of its own
    factual top 20 and one of its corrected top 20 (so that kept, gained and lost hits exist whatever the draw)"""
    from macr_amd.evaluator import Evaluator
    d = request.param
    rs = np.random.RandomState(d)
    n_users, N = 320, 500
    P = (rs.standard_normal((n_users, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    pop = rs.standard_normal(N).astype(np.float32)
    Q += (pop * 0.5)[:, None] * np.sign(P.mean(0, keepdims=True))
    w = (np.sign(P.mean(0)) * 0.4 + rs.standard_normal(d) * 0.1).astype(np.float32)
    wu = (rs.standard_normal(d) * 0.3).astype(np.float32)
    uid_np = rs.permutation(n_users)[:300].astype(np.int32)
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(300)]
    gt = [sorted(set(rs.randint(0, N, rs.randint(0, 6)).tolist())) for _ in range(300)]
    t = dict(P=dev(P), Q=dev(Q), w=dev(w), wu=dev(wu), uid=dev(uid_np))
    sig_i = ops.branch_sigmoid(t["Q"], t["w"])
    sig_u = ops.branch_sigmoid(t["P"], t["wu"], t["uid"])
    scores = {ops.SCORE_NORMAL: ops.score_matrix(ops.SCORE_NORMAL, t["P"], t["uid"], t["Q"]).cpu().numpy(),
              ops.SCORE_RUBI_BOTH: ops.score_matrix(ops.SCORE_RUBI_BOTH, t["P"], t["uid"], t["Q"], sig_u, sig_i, C).cpu().numpy(),
              ops.SCORE_RUBI: ops.score_matrix(ops.SCORE_RUBI, t["P"], t["uid"], t["Q"], None, sig_i, C).cpu().numpy()}
    lists = {kind: item_acc_ref.rank_outside_train(s, mask, K) for kind, s in scores.items()}
    for u in range(0, 300, 7):
        gt[u] = sorted(set(gt[u]) | {int(lists[ops.SCORE_NORMAL][u, u % K]), int(lists[ops.SCORE_RUBI_BOTH][u, (u + 3) % K])})
    return dict(t, mask=mask, gt=gt, N=N, scores=scores, lists=lists, sig=(sig_u, sig_i), ev=Evaluator(mask, gt, N, "cuda"))


@pytest.mark.parametrize("kind_name", ["SCORE_RUBI_BOTH", "SCORE_RUBI"])
def test_list_shift_and_depth_against_a_host_full_sort(ops, model, kind_name):
    m, kind, ev = model, getattr(ops, kind_name), model["ev"]
    base_ids, here_ids = m["lists"][ops.SCORE_NORMAL], m["lists"][kind]
    want_pu, want_ent, want_left = R.list_shift(base_ids, here_ids, m["gt"], K, m["N"])
    assert (want_pu[:, 3] < K).sum() > 200 and (want_ent >= 0).sum() > 300           # c is large enough: the lists differ
    group_np = (np.arange(m["N"]) * 7 % 6).astype(np.int32)
    args = (kind, m["P"], m["uid"], m["Q"])
    pu, ent, left, ec, lc = ev.list_shift(*args, K, m["w"], m["wu"], C, group_of=group_np, n_groups=6)
    assert pu.dtype == ent.dtype == left.dtype == torch.int32
    assert np.array_equal(pu.cpu().numpy(), want_pu)
    assert np.array_equal(ent.cpu().numpy(), want_ent) and np.array_equal(left.cpu().numpy(), want_left)
    for (rec, hit, sums), ids in ((ec, want_ent), (lc, want_left)):
        want_rec, want_hit = item_acc_ref.item_counts(ids, m["gt"], K, m["N"])
        assert np.array_equal(rec.cpu().numpy(), want_rec) and np.array_equal(hit.cpu().numpy(), want_hit)
        assert np.array_equal(sums.cpu().numpy(), item_acc_ref.group_sums(group_np, want_rec, want_hit, 6))
    gained, lost = int(ec[1].sum()), int(lc[1].sum())
    assert gained == int((want_pu[:, 6] - want_pu[:, 7]).sum()) and lost == int((want_pu[:, 5] - want_pu[:, 7]).sum())
    if kind == ops.SCORE_RUBI_BOTH:
        assert gained > 0 and lost > 0 and want_pu[:, 7].sum() > 0
    # without groups: no group sums; another base: a ranking against itself is identical
    assert ev.list_shift(*args, K, m["w"], m["wu"], C)[3][2] is None
    same = ev.list_shift(*args, K, m["w"], m["wu"], C, base_kind=kind, base_c=C)
    assert (same[0][:, 3] == K).all() and (same[1] == -1).all() and (same[2] == -1).all()
    # the depths: exact positions in the full rankings
    pos_e, pos_l = ev.shift_depth(*args, ent, left, m["w"], m["wu"], C)
    want_e = R.full_positions(m["scores"][ops.SCORE_NORMAL], m["mask"], want_ent)
    want_l = R.full_positions(m["scores"][kind], m["mask"], want_left)
    assert pos_e.dtype == torch.int32 and np.array_equal(pos_e.cpu().numpy(), want_e) and np.array_equal(pos_l.cpu().numpy(), want_l)
    ptr, _ = R.pairs_of(want_ent)
    full_base = np.repeat(want_pu[:, 0] == K, np.diff(ptr))
    assert full_base.any() and (want_e[full_base] >= K).all() and (pos_e.cpu().numpy()[full_base] >= K).all()
    assert (want_l >= K).all()                                                          # (every here row of this model is full)


def test_rank_positions_without_pairs_is_unchanged(ops, model):
    m, ev = model, model["ev"]
    sig_u, sig_i = m["sig"]
    got = ev.rank_positions(ops.SCORE_RUBI_BOTH, m["P"], m["uid"], m["Q"], m["w"], m["wu"], C)
    direct = ops.rank_positions(ops.SCORE_RUBI_BOTH, m["P"], m["uid"], m["Q"], ev.gt, sig_u, sig_i, C, ev.mask, n_pairs=ev.n_gt)
    assert got.shape == (ev.n_gt,) and torch.equal(got, direct)
    gt_rows = np.full((300, 8), -1, dtype=np.int64)
    for u, row in enumerate(m["gt"]):
        gt_rows[u, :len(row)] = row
    assert np.array_equal(got.cpu().numpy(), R.full_positions(m["scores"][ops.SCORE_RUBI_BOTH], m["mask"], gt_rows))
    # and with the ground truth handed in as pairs: the same numbers
    ptr, idx = R.pairs_of(gt_rows)
    assert torch.equal(ev.rank_positions(ops.SCORE_RUBI_BOTH, m["P"], m["uid"], m["Q"], m["w"], m["wu"], C,
                                         pairs=(dev(ptr), dev(idx), len(idx))), got)
    # no pairs at all
    none = ev.rank_positions(ops.SCORE_NORMAL, m["P"], m["uid"], m["Q"],
                             pairs=(torch.zeros(301, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), 0))
    assert none.numel() == 0


def test_metrics_are_the_same_with_a_list_shift_in_between(ops, model):
    from macr_amd.evaluator import Evaluator
    m = model
    args = (ops.SCORE_RUBI_BOTH, m["P"], m["uid"], m["Q"])
    plain, mixed = Evaluator(m["mask"], m["gt"], m["N"], "cuda"), Evaluator(m["mask"], m["gt"], m["N"], "cuda")
    want = [plain.test_mf(*args, [5, K], m["w"], m["wu"], C) for _ in range(3)]
    got = [mixed.test_mf(*args, [5, K], m["w"], m["wu"], C)]
    first = mixed.list_shift(*args, K, m["w"], m["wu"], C)
    got.append(mixed.test_mf(*args, [5, K], m["w"], m["wu"], C))
    second = mixed.list_shift(*args, K, m["w"], m["wu"], C)
    got.append(mixed.test_mf(*args, [5, K], m["w"], m["wu"], C))
    for a, b in zip(want, got):
        # (bytes: queries with an empty ground truth make the mean recall nan, and nan != nan)
        assert sorted(a) == sorted(b) and all(a[key].tobytes() == b[key].tobytes() for key in a)
    assert want[0]["hit_ratio"][-1] > 0
    assert all(torch.equal(x, y) for x, y in zip(first[:3], second[:3]))
    assert mixed._base_evaluator() is mixed._base_evaluator() and mixed._base_evaluator() is not mixed
