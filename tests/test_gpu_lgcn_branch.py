"""LightGCN's item-branch losses and rankings on the HIP path (-m gpu): `--loss bce1` (MACR_LOSS_RUBIBCE on the propagated rows,
LightGCN.py:432-461), `--loss bce2` (MACR_LOSS_RUBIBCE_EGO: the branch on the ego rows, :463-493), `--test rubi1 / rubi2`
(:442 / :473).  One step against the reference's graph code (G12), trajectories against the float64 restatement of
tests/lgcn_branch_ref.py, the rankings against the oracle, the model, the session shim and the CLIs."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bpr_ref
import lgcn_branch_ref
import oracle
from helpers import GOLD, REPO, golden_npz_parts

pytestmark = pytest.mark.gpu

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 1024


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def hyper(ops):
    return ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)


def kinds(ops):
    return {"bce1": ops.LOSS_RUBIBCE, "bce2": ops.LOSS_RUBIBCE_EGO}


# ----------------------------------------------------------------------------- one step against the reference's graph
@pytest.mark.parametrize("loss", ["bce1", "bce2"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_step_matches_reference_graph(ops, tag, loss):
    G10 = golden_npz_parts("G10_model_steps")
    with np.load(os.path.join(GOLD, "G12_lgcn_item_branch.npz")) as z:
        G = {k: z[k] for k in z.files}
    g = lambda k: G10["lgcn_%s/%s" % (tag, k)]
    P, Q = g("P"), g("Q")
    w0, wu0 = g("w").reshape(-1), g("wu").reshape(-1)
    adj = ops.CSR(dev(g("indptr"), torch.int32), dev(g("indices"), torch.int32), dev(g("data"))).build_spmm_plan()
    state = ops.LGCNState(dev(np.concatenate([P, Q])), P.shape[0], Q.shape[0], dev(w0), dev(wu0), adj, 2, hyper(ops), len(g("u")))
    got = state.step(kinds(ops)[loss], dev(g("u"), torch.int32), dev(g("i"), torch.int32), dev(g("j"), torch.int32)).cpu().numpy()
    for dt in ("f32", "f64"):
        want = [float(G["lgcn_%s/%s/%s/%s" % (tag, loss, dt, k)]) for k in ("loss", "mf_loss", "emb_loss")]
        np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=dt)
    pre = "lgcn_%s/%s/f64/" % (tag, loss)
    dT = np.concatenate([G[pre + "dP"], G[pre + "dQ"]])
    np.testing.assert_allclose(state.mT.cpu().numpy() / 0.1, dT, rtol=5e-4, atol=2e-6 * np.abs(dT).max())
    dw = G[pre + "dw"].reshape(-1)
    np.testing.assert_allclose(state.mw.cpu().numpy() / 0.1, dw, rtol=5e-4, atol=2e-6 * np.abs(dw).max())
    assert not np.array_equal(state.w.cpu().numpy(), w0)
    assert np.array_equal(state.wu.cpu().numpy(), wu0)                  # w_user: no gradient, TF leaves it alone
    assert not state.mwu.cpu().numpy().any() and not state.vwu.cpu().numpy().any()


# ----------------------------------------------------------------------------- trajectories against the restatement
def lgcn_graph(seed, n_users, n_items, n_inter, asym):
    import scipy.sparse as sp
    rs = np.random.RandomState(seed)
    R = sp.coo_matrix((np.ones(n_inter), (rs.randint(0, n_users, n_inter), rs.zipf(1.3, n_inter) % n_items)),
                      shape=(n_users, n_items)).tocsr()
    R = (R + sp.csr_matrix((np.ones(n_users), (np.arange(n_users), rs.randint(0, n_items, n_users))), shape=R.shape)).tocsr()
    R = (R + sp.csr_matrix((np.ones(n_items), (rs.randint(0, n_users, n_items), np.arange(n_items))), shape=R.shape)).tocsr()
    R.data[:] = 1.0
    A = sp.bmat([[None, R], [R.T, None]]).tocsr()
    deg = np.asarray(A.sum(1)).ravel()
    M = sp.diags(1.0 / deg).dot(A) if asym else sp.diags(deg ** -0.5).dot(A).dot(sp.diags(deg ** -0.5))
    M = M.tocsr().astype(np.float32)
    M.sort_indices()
    return M, rs


def batch(rs, n_users, n_items, B, zipf=True):
    pos = rs.zipf(1.3, B) % n_items if zipf else rs.randint(0, n_items, B)
    return rs.randint(0, n_users, B).astype(np.int32), pos.astype(np.int32), rs.randint(0, n_items, B).astype(np.int32)


def run_trajectory(ops, loss, asym, n_layers, d, dense, n_users=500, n_items=300, B=512, steps=20, seed=0, zipf=True):
    M, rs = lgcn_graph(seed + 7 * n_layers + d + asym, n_users, n_items, 4000, asym)
    Mt = M.T.tocsr()
    Mt.sort_indices()
    T0 = (rs.standard_normal((n_users + n_items, d)) * 0.1).astype(np.float32)
    w0 = (rs.standard_normal(d) * 0.3).astype(np.float32)
    adj = ops.CSR.from_scipy(M, "cuda")
    adj_t = ops.CSR.from_scipy(Mt, "cuda") if asym else None
    state = ops.LGCNState(dev(T0), n_users, n_items, dev(w0), dev(w0), adj, n_layers, hyper(ops), B, adj_t=adj_t)
    M64, Mt64 = M.astype(np.float64), Mt.astype(np.float64)
    ref = bpr_ref.Adam([T0, w0], LR)
    for t in range(steps):
        u, i, j = batch(rs, n_users, n_items, B, zipf)
        want = lgcn_branch_ref.lgcn_item_branch(M64, ref.params[0], ref.params[1], n_users, n_layers, u, i, j, ALPHA, DECAY, BS,
                                                ego=loss == "bce2", At=Mt64)
        got = state.step(kinds(ops)[loss], dev(u), dev(i), dev(j), dense_layers=dense).cpu().numpy()
        np.testing.assert_allclose(got, want[:3], rtol=5e-5, err_msg="step %d" % t)
        ref.step([want[3], want[4]])
    return state, ref, (M64, Mt64, rs, n_users, n_items, B)


@pytest.mark.parametrize("loss", ["bce1", "bce2"])
@pytest.mark.parametrize("d,dense", [(32, False), (64, False), (64, True), (128, True), (256, False)])
@pytest.mark.parametrize("n_layers", [1, 2, 3])
@pytest.mark.parametrize("asym", [False, True])
def test_twenty_step_trajectory(ops, loss, asym, n_layers, d, dense):
    steps = 20
    state, ref, (M64, Mt64, rs, n_users, n_items, B) = run_trajectory(ops, loss, asym, n_layers, d, dense, steps=steps)
    for got, want, name in ((state.T, ref.params[0], "T"), (state.w, ref.params[1], "w")):
        diff = np.abs(got.cpu().numpy() - want)
        assert diff.max() <= 2e-3 * LR * steps and diff.mean() <= 1e-4 * LR * steps, (name, diff.max(), diff.mean())
    assert not state.mwu.cpu().numpy().any() and not state.vwu.cpu().numpy().any()      # w_user untouched
    # loss-only pass: the losses of the batch as of now, nothing written
    u, i, j = batch(rs, n_users, n_items, B)
    want = lgcn_branch_ref.lgcn_item_branch(M64, state.T.cpu().numpy(), state.w.cpu().numpy(), n_users, n_layers, u, i, j,
                                            ALPHA, DECAY, BS, ego=loss == "bce2", At=Mt64)
    before = {n: getattr(state, n).clone() for n in ("T", "w", "wu", "mT", "vT", "mw", "vw", "mwu", "vwu", "adam_pow")}
    got = state.step(kinds(ops)[loss], dev(u), dev(i), dev(j), loss_only=True, dense_layers=dense).cpu().numpy()
    np.testing.assert_allclose(got, want[:3], rtol=5e-5)
    for n, v in before.items():
        assert torch.equal(getattr(state, n), v), n


@pytest.mark.parametrize("loss", ["bce1", "bce2"])
def test_staged_path_trajectory_and_determinism(ops, loss):
    """B > 8192: the staged gradient path (the branch scalars staged and summed in list order with the rows).  Five steps
    against the restatement; then one step from the same state twice: the table's gradient (the first moment of T) is the
    same bits both times (uniform batch: no row has references in more than two 16-reference chunks, whose two sums add
    the same either way round).  w's gradient meets in a few partial rows by atomics, as for bceboth: equal up to order."""
    state, ref, _ = run_trajectory(ops, loss, False, 2, 64, False, n_users=6000, n_items=3000, B=12000, steps=5, seed=3)
    for got, want in ((state.T, ref.params[0]), (state.w, ref.params[1])):
        diff = np.abs(got.cpu().numpy() - want)
        assert diff.max() <= 2e-3 * LR * 5 and diff.mean() <= 1e-4 * LR * 5, (diff.max(), diff.mean())
    M, rs = lgcn_graph(11, 6000, 20000, 20000, False)
    T0 = (rs.standard_normal((26000, 64)) * 0.1).astype(np.float32)
    w0 = (rs.standard_normal(64) * 0.3).astype(np.float32)
    u, i, j = batch(rs, 6000, 20000, 12000, zipf=False)
    adj = ops.CSR.from_scipy(M, "cuda")
    runs = []
    for _ in range(2):
        st = ops.LGCNState(dev(T0), 6000, 20000, dev(w0), dev(w0), adj, 2, hyper(ops), 12000)
        losses = st.step(kinds(ops)[loss], dev(u), dev(i), dev(j)).clone()
        runs.append((losses, st.mT.clone(), st.mw.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    torch.testing.assert_close(runs[0][2], runs[1][2], rtol=1e-5, atol=1e-9)


# ----------------------------------------------------------------------------- the model
def _lgcn(ops, n_users=400, n_items=250):
    from macr_amd.lightgcn import LightGCN
    M, _ = lgcn_graph(5, n_users, n_items, 3000, False)
    args = types.SimpleNamespace(adj_type="pre", alg_type="lightgcn", lr=1e-3, embed_size=64, batch_size=256,
                                 layer_size="[64,64]", regs="[1e-5]", verbose=0, Ks="[20]", alpha=1e-2, beta=1e-3,
                                 dataset="synthetic", node_dropout_flag=0)
    return LightGCN(dict(n_users=n_users, n_items=n_items, norm_adj=M), args, seed=3)


@pytest.mark.parametrize("loss", ["bce1", "bce2"])
def test_session_shim_matches_fast_path(ops, loss):
    from macr_amd.mf import Session
    a, b = _lgcn(ops), _lgcn(ops)
    sess = Session(a)
    rs = np.random.RandomState(1)
    u = rs.choice(400, 256, replace=False).tolist(); i = rs.randint(0, 250, 256).tolist(); j = rs.randint(0, 250, 256).tolist()
    sfx = "_two_" + loss
    f = [getattr(a, n + sfx) for n in ("opt", "loss", "mf_loss", "emb_loss", "reg_loss")]
    _, l, mf, emb, reg = sess.run(f, feed_dict={a.users: u, a.pos_items: i, a.neg_items: j})
    direct = b.train_step(b.kind_of(loss), b.to_device_batch(u, i, j)).cpu().numpy()
    np.testing.assert_allclose([l, mf, emb], direct, rtol=1e-6)
    assert float(np.asarray(reg).ravel()[0]) == 0.0
    torch.testing.assert_close(a.T, b.T, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(a.w, b.w, rtol=1e-5, atol=1e-7)
    # the ranking fetches: (y - c) sig(e_i . w), e_i propagated (rubi1) or ego (rubi2)
    a.update_c(sess, 0.7)
    users = list(range(30))
    r1, r2 = sess.run([a.rubi_ratings1, a.rubi_ratings2], feed_dict={a.users: users})
    ua, ia = a.propagated()
    y = (ua[:30] @ ia.T).cpu().numpy().astype(np.float64) - 0.7
    for r, rows in ((r1, ia), (r2, a.T[400:])):
        sig = 1.0 / (1.0 + np.exp(-(rows @ a.w).cpu().numpy().astype(np.float64)))
        np.testing.assert_allclose(r, y * sig[None, :], rtol=1e-4, atol=1e-6)


def test_branch_states_exist_only_once_used_and_survive_a_checkpoint(ops):
    g = _lgcn(ops)
    rs = np.random.RandomState(2)
    mk = lambda: g.to_device_batch(rs.choice(400, 64), rs.randint(0, 250, 64), rs.randint(0, 250, 64))
    g.train_step(ops.LOSS_NORMALBCE, mk())
    assert ops.LOSS_RUBIBCE not in g._opt and ops.LOSS_RUBIBCE_EGO not in g._opt
    assert not any(k.startswith("opt%d." % ops.LOSS_RUBIBCE_EGO) for k in g.state_dict())
    for _ in range(3):
        g.train_step(ops.LOSS_RUBIBCE_EGO, mk())
    assert g._opt[ops.LOSS_RUBIBCE_EGO].T is g.T
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in g.state_dict().items()}
    h = _lgcn(ops)
    h.load_state_dict(sd)
    batch = mk()
    la, lb = g.train_step(ops.LOSS_RUBIBCE_EGO, batch).cpu().numpy(), h.train_step(ops.LOSS_RUBIBCE_EGO, batch).cpu().numpy()
    assert np.array_equal(la, lb)
    assert torch.equal(g.T, h.T) and torch.equal(g.w, h.w)


# ----------------------------------------------------------------------------- rankings
def random_mask(rs, U, N, per):
    return [sorted(set(rs.randint(0, N, per).tolist())) for _ in range(U)]


@pytest.mark.parametrize("filt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("ego", [False, True])
def test_rubi_rankings_bit_exact(ops, monkeypatch, filt, ego):
    """rubi1 / rubi2 through the Evaluator (one-launch prologue; under f16 the prologue with the fp16 copies) against the
    oracle given sig_i of the branch table; seeded (second call) and unseeded"""
    from macr_amd.evaluator import Evaluator
    monkeypatch.setenv("MACR_EVAL_FILTER", filt)
    rs = np.random.RandomState(11 + ego)
    n_users, N, d, U, K, c = 700, 20000, 64, 300, 20, 0.4
    P = (rs.standard_normal((n_users, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    Q0 = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)      # the "ego" rows: a table of their own
    w = (rs.standard_normal(d) * 0.3).astype(np.float32)
    uid = rs.permutation(n_users)[:U].astype(np.int32)
    mask = random_mask(rs, U, N, 12)
    ev = Evaluator(mask, [[0]] * U, N, "cuda")
    branch = Q0 if ego else Q
    sig_i = ops.branch_sigmoid(dev(branch), dev(w)).cpu().numpy()
    mptr, midx = oracle.csr_from_lists(mask)
    want_v, want_i, want_c = oracle.score_topk(ops.SCORE_RUBI, P[uid], Q, K, None, sig_i, c, (mptr, midx))
    for _ in range(2):
        gv, gi, gc = ev.rank(ops.SCORE_RUBI, dev(P), dev(uid), dev(Q), K, dev(w), None, c, branch=dev(Q0) if ego else None)
        assert np.array_equal(gi.cpu().numpy(), want_i)
        assert np.array_equal(gv.cpu().numpy().view(np.uint32), want_v.view(np.uint32))


def test_rubi2_sweep_equals_per_c_runs_and_item_shards_merge(ops):
    from macr_amd.evaluator import Evaluator
    rs = np.random.RandomState(5)
    n_users, N, d, U, Ks = 500, 9000, 64, 200, (5, 20)
    P = dev((rs.standard_normal((n_users, d)) * 0.5).astype(np.float32))
    Q = dev((rs.standard_normal((N, d)) * 0.5).astype(np.float32))
    Q0 = dev((rs.standard_normal((N, d)) * 0.5).astype(np.float32))
    w = dev((rs.standard_normal(d) * 0.3).astype(np.float32))
    uid = dev(rs.permutation(n_users)[:U].astype(np.int32))
    mask = random_mask(rs, U, N, 10)
    gt = [sorted(set(rs.randint(0, N, 5).tolist())) for _ in range(U)]
    ev = Evaluator(mask, gt, N, "cuda")
    cs = [0.0, 0.3, 1.0, 2.5, 4.0]
    sweep = ev.test_lgcn_sweep(ops.SCORE_RUBI, P, uid, Q, Ks, w, None, cs, branch=Q0)
    for c, r in zip(cs, sweep):
        one = Evaluator(mask, gt, N, "cuda").test_lgcn(ops.SCORE_RUBI, P, uid, Q, Ks, w, None, c, branch=Q0)
        for k in ("hr", "recall", "ndcg"):
            np.testing.assert_array_equal(r[k], one[k])
    # two item-shard ranges, each ranking its rows of Q and of the branch table, merge to the unsharded ranking
    full_v, full_i, _ = Evaluator(mask, gt, N, "cuda").rank(ops.SCORE_RUBI, P, uid, Q, 20, w, None, 1.0, branch=Q0)
    parts = []
    for lo, hi in ((0, 4000), (4000, N)):
        e = Evaluator(mask, gt, N, "cuda")
        e.local_items_range = (lo, hi)
        parts.append(e.rank_local(ops.SCORE_RUBI, P, uid, Q[lo:hi].contiguous(), 20, w, None, 1.0, Q0[lo:hi].contiguous()))
    mv, mi, _ = ops.topk_merge(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    assert torch.equal(mi, full_i) and torch.equal(mv, full_v)


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


@pytest.mark.parametrize("script,loss,test", [("LightGCN.py", "bce1", "rubi1"), ("LightGCN.py", "bce2", "rubi2"),
                                              ("LightGCN_tune.py", "bce2", "rubi2")])
def test_lightgcn_cli_item_branch(tmp_path, script, loss, test):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    out = _run([os.path.join(REPO, "macr_lightgcn", script), "--data_path", str(tmp_path / "data") + "/", "--dataset", "tiny_data",
                "--verbose", "1", "--layer_size", "[64,64]", "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0",
                "--epoch", "4", "--log_interval", "2", "--weights_path", str(tmp_path) + "/", "--saveID", loss, "--loss", loss,
                "--test", test, "--c", "0.5", "--start", "0", "--end", "1", "--step", "3", "--sampler", "device"], str(tmp_path))
    lines = [l for l in out.splitlines() if l.startswith("c:")]
    assert lines and all("hit=[" in l and "ndcg=[" in l for l in lines), out
    if script == "LightGCN_tune.py":
        assert len(lines) % 3 == 0, out
