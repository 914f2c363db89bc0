"""Evaluator.list_calibration (MACR_CALIBRATION_REPORT) on a small random MF model against a host full sort of macr_score_matrix's
output under the project's tie rule (score descending, ties by ascending id, train items excluded) and the plain-loop
restatement (tests/calibration_ref.py).  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

import calibration_ref as R
import item_acc_ref

pytestmark = pytest.mark.gpu

K = 20
C = 0.7
G = 6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def model(ops):
    """300 query users of 320 x 500 items, d = 64, item rows with a popularity direction the item branch picks up, hand-set w
    and w_user; train lists of 0 .. 30 items (user 3: none), ground truth of 0 .. 6 items plus, for every seventh user, one
    item of its factual and one of its corrected top 20; train counts as weights, groups cut from them"""
    d = 64
    rs = np.random.RandomState(d)
    n_users, N = 320, 500
    P = (rs.standard_normal((n_users, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    pop = rs.standard_normal(N).astype(np.float32)
    Q += (pop * 0.5)[:, None] * np.sign(P.mean(0, keepdims=True))
    w = (np.sign(P.mean(0)) * 0.4 + rs.standard_normal(d) * 0.1).astype(np.float32)
    wu = (rs.standard_normal(d) * 0.3).astype(np.float32)
    uid_np = rs.permutation(n_users)[:300].astype(np.int32)
    mask = [sorted(rs.choice(N, rs.randint(1, 30), replace=False).tolist()) for _ in range(300)]
    mask[3] = []
    gt = [sorted(set(rs.randint(0, N, rs.randint(0, 6)).tolist())) for _ in range(300)]
    weight = np.zeros(N, dtype=np.int32)
    for row in mask:
        weight[row] += 1
    group_of = np.minimum(weight // 4, G - 1).astype(np.int32)
    t = dict(P=dev(P), Q=dev(Q), w=dev(w), wu=dev(wu), uid=dev(uid_np))
    sig_i = ops.branch_sigmoid(t["Q"], t["w"])
    sig_u = ops.branch_sigmoid(t["P"], t["wu"], t["uid"])
    scores = {ops.SCORE_NORMAL: ops.score_matrix(ops.SCORE_NORMAL, t["P"], t["uid"], t["Q"]).cpu().numpy(),
              ops.SCORE_RUBI_BOTH: ops.score_matrix(ops.SCORE_RUBI_BOTH, t["P"], t["uid"], t["Q"], sig_u, sig_i, C).cpu().numpy()}
    lists = {kind: item_acc_ref.rank_outside_train(s, mask, K) for kind, s in scores.items()}
    for u in range(0, 300, 7):
        gt[u] = sorted(set(gt[u]) | {int(lists[ops.SCORE_NORMAL][u, u % K]), int(lists[ops.SCORE_RUBI_BOTH][u, (u + 3) % K])})
    want = {kind: R.group_hist(ids, group_of, G, N, gt, weight, k=K) for kind, ids in lists.items()}
    profile = R.group_hist(mask, group_of, G, N, item_weight=weight)
    return dict(t, mask=mask, gt=gt, N=N, scores=scores, lists=lists, want=want, profile=profile, weight=weight, group_of=group_of)


def host(t):
    return [None if x is None else x.cpu().numpy() for x in t]


def same(got, want):
    got = host(got)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), np.argwhere(g != w)[:5]


def call(ev, m, kind, **kw):
    return ev.list_calibration(kind, m["P"], m["uid"], m["Q"], K, m["w"], m["wu"], C, group_of=m["group_of"], n_groups=G,
                               item_weight=m["weight"], **kw)


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_list_calibration_against_a_host_full_sort(ops, model, kind_name):
    from macr_amd.evaluator import Evaluator
    m, kind = model, getattr(ops, kind_name)
    ev = Evaluator(m["mask"], m["gt"], m["N"], "cuda")
    profile, here, base = call(ev, m, kind)
    assert base is None
    same(profile, (m["profile"][0], m["profile"][2]))
    same(here, m["want"][kind])
    assert m["want"][kind][1].sum() > 0 and tuple(m["profile"][2][3]) == (0, 0)            # hits exist; user 3 has no profile
    # the profile is computed once per evaluator and group table, and kept
    profile2, here2, base2 = call(ev, m, kind, with_base=True)
    assert profile2[0] is profile[0] and profile2[1] is profile[1]
    same(here2, m["want"][kind])
    same(base2, m["want"][ops.SCORE_NORMAL])
    if kind != ops.SCORE_NORMAL:
        assert not np.array_equal(m["want"][kind][0], m["want"][ops.SCORE_NORMAL][0])      # c is large enough: the mixes differ
    # another group table: counted anew
    other = (m["group_of"] + 1) % G
    profile3, here3, _ = ev.list_calibration(kind, m["P"], m["uid"], m["Q"], K, m["w"], m["wu"], C, group_of=other, n_groups=G)
    assert profile3[0] is not profile[0]
    same(profile3, [x for x in R.group_hist(m["mask"], other, G, m["N"]) if x is not None])
    same(here3, R.group_hist(m["lists"][kind], other, G, m["N"], m["gt"], k=K))
    with pytest.raises(ops.MacrError):
        ev.list_calibration(kind, m["P"], m["uid"], m["Q"], K, m["w"], m["wu"], C)


def test_the_report_of_the_device_counts_is_the_restatements(ops, model):
    from macr_amd import calibration
    from macr_amd.evaluator import Evaluator
    m = model
    ev = Evaluator(m["mask"], m["gt"], m["N"], "cuda")
    profile, here, base = call(ev, m, ops.SCORE_RUBI_BOTH, with_base=True)
    sizes = np.diff(ev.gt.ptr.cpu().numpy())
    assert np.array_equal(sizes, [len(g) for g in m["gt"]])
    got = calibration.summarize(host(profile), host(here), sizes, K, host(base))
    want = R.summarize((m["profile"][0], m["profile"][2]), m["want"][ops.SCORE_RUBI_BOTH], sizes, K, m["want"][ops.SCORE_NORMAL])
    assert got["users"] == want["users"] == 299 and got["skipped"] == 1
    for a, b in ((got, want), (got["base"], want["base"])):
        for key in ("js", "tv", "gap_profile", "gap_list", "lift", "recall"):
            assert abs(a[key] - b[key]) <= 1e-12, key
            for t in R.TASTE:
                assert a["taste"][t]["users"] == b["taste"][t]["users"] and abs(a["taste"][t][key] - b["taste"][t][key]) <= 1e-12, (t, key)


def test_the_main_evaluators_state_is_what_a_call_without_base_leaves(ops, model):
    from macr_amd.evaluator import Evaluator
    m = model
    args = (ops.SCORE_RUBI_BOTH, m["P"], m["uid"], m["Q"])
    plain, mixed = Evaluator(m["mask"], m["gt"], m["N"], "cuda"), Evaluator(m["mask"], m["gt"], m["N"], "cuda")
    for rep in range(2):
        want = plain.test_mf(*args, [5, K], m["w"], m["wu"], C)
        got = mixed.test_mf(*args, [5, K], m["w"], m["wu"], C)
        assert sorted(want) == sorted(got) and all(want[key].tobytes() == got[key].tobytes() for key in want)
        call(plain, m, ops.SCORE_RUBI_BOTH)
        call(mixed, m, ops.SCORE_RUBI_BOTH, with_base=True)
        assert plain._policy == mixed._policy and set(plain._seeds) == set(mixed._seeds)
        assert all(torch.equal(plain._seeds[key], mixed._seeds[key]) for key in plain._seeds)
        assert set(plain._graphs) == set(mixed._graphs) and plain._last_depth == mixed._last_depth
    assert mixed._base_evaluator() is not mixed and plain._base is None


def test_a_strided_item_shard_gives_the_same_arrays(ops, model):
    """rank 1 of 3 of an interleaved item table (set_local_items), played alone: the profile is the one of the whole train lists
    (global ids), the lists are the host's full sort over the shard's items, for `here` and for the base evaluator alike"""
    from macr_amd.evaluator import Evaluator
    from macr_amd.sharded_train import Owned
    m = model
    own = Owned(m["N"], 1, 3)
    assert own.stride == 3
    mine = own.lo + own.stride * np.arange(own.n)
    ev = Evaluator(m["mask"], m["gt"], m["N"], "cuda")
    ev.set_local_items(own)
    profile, here, base = ev.list_calibration(ops.SCORE_RUBI_BOTH, m["P"], m["uid"], dev(m["Q"].cpu().numpy()[mine]), K, m["w"], m["wu"], C,
                                              group_of=m["group_of"], n_groups=G, item_weight=m["weight"], with_base=True)
    same(profile, (m["profile"][0], m["profile"][2]))
    where = {int(g): l for l, g in enumerate(mine)}
    local_mask = [[where[g] for g in row if g in where] for row in m["mask"]]
    for got, kind in ((here, ops.SCORE_RUBI_BOTH), (base, ops.SCORE_NORMAL)):
        local = item_acc_ref.rank_outside_train(m["scores"][kind][:, mine], local_mask, K)
        ids = np.where(local >= 0, own.lo + own.stride * local, -1).astype(np.int32)
        same(got, R.group_hist(ids, m["group_of"], G, m["N"], m["gt"], m["weight"], k=K))
