"""BPR losses on the HIP path (-m gpu): MF `--train normal` (MACR_LOSS_BPR, macr_mf/model.py:264-275) and LightGCN
`--loss bpr` (MACR_LOSS_BPR_LGCN, LightGCN.py:398-413).  One step against the reference's graph code (G11), multi-step
trajectories against the float64 restatement of tests/bpr_ref.py, the entry points around them, the models and the CLIs."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import bpr_ref
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


def close_grad(got, want, name, rtol):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=2e-6 * np.abs(want).max() + 1e-12, err_msg=name)


def g11():
    with np.load(os.path.join(GOLD, "G11_bpr_steps.npz")) as z:
        return {k: z[k] for k in z.files}


def hyper(ops):
    return ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)


# ----------------------------------------------------------------------------- one step against the reference's graph
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_mf_bpr_step_matches_reference_graph(ops, tag):
    G10, G = golden_npz_parts("G10_model_steps"), g11()
    g = lambda k: G10["mf_%s/%s" % (tag, k)]
    w0, wu0 = g("w").reshape(-1), g("wu").reshape(-1)
    state = ops.MFState(dev(g("P")), dev(g("Q")), dev(w0), dev(wu0), hyper(ops), len(g("u")))
    got = state.step(ops.LOSS_BPR, dev(g("u"), torch.int32), dev(g("i"), torch.int32), dev(g("j"), torch.int32)).cpu().numpy()
    for dt in ("f32", "f64"):
        want = [float(G["mf_%s/bpr/%s/%s" % (tag, dt, k)]) for k in ("loss", "mf_loss", "reg_loss")]
        np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=dt)
    pre = "mf_%s/bpr/f64/" % tag
    close_grad(state.mP.cpu().numpy() / 0.1, G[pre + "dP"], "dP", 2e-4)
    close_grad(state.mQ.cpu().numpy() / 0.1, G[pre + "dQ"], "dQ", 2e-4)
    # `opt` trains the `parameter` scope (:52-57): w, w_user and their slots bitwise untouched
    assert np.array_equal(state.w.cpu().numpy(), w0) and np.array_equal(state.wu.cpu().numpy(), wu0)
    for s in (state.mw, state.vw, state.mwu, state.vwu):
        assert not s.cpu().numpy().any()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_lightgcn_bpr_step_matches_reference_graph(ops, tag):
    G10, G = golden_npz_parts("G10_model_steps"), g11()
    g = lambda k: G10["lgcn_%s/%s" % (tag, k)]
    P, Q = g("P"), g("Q")
    w0, wu0 = g("w").reshape(-1), g("wu").reshape(-1)
    adj = ops.CSR(dev(g("indptr"), torch.int32), dev(g("indices"), torch.int32), dev(g("data"))).build_spmm_plan()
    state = ops.LGCNState(dev(np.concatenate([P, Q])), P.shape[0], Q.shape[0], dev(w0), dev(wu0), adj, 2, hyper(ops), len(g("u")))
    got = state.step(ops.LOSS_BPR_LGCN, dev(g("u"), torch.int32), dev(g("i"), torch.int32), dev(g("j"), torch.int32)).cpu().numpy()
    for dt in ("f32", "f64"):
        want = [float(G["lgcn_%s/bpr/%s/%s" % (tag, dt, k)]) for k in ("loss", "mf_loss", "emb_loss")]
        np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=dt)
    pre = "lgcn_%s/bpr/f64/" % tag
    close_grad(state.mT.cpu().numpy() / 0.1, np.concatenate([G[pre + "dP"], G[pre + "dQ"]]), "dT", 5e-4)
    assert np.array_equal(state.w.cpu().numpy(), w0) and np.array_equal(state.wu.cpu().numpy(), wu0)
    for s in (state.mw, state.vw, state.mwu, state.vwu):
        assert not s.cpu().numpy().any()


# ----------------------------------------------------------------------------- MF trajectories
def mf_problem(seed, n_users, n_items, d, scale=0.3):
    rs = np.random.RandomState(seed)
    P = (rs.standard_normal((n_users, d)) * scale).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * scale).astype(np.float32)
    w = (rs.standard_normal(d) * 0.3).astype(np.float32)
    return P, Q, w, rs


def mf_batch(rs, n_users, n_items, B):
    u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
    i = rs.randint(0, n_items, B).astype(np.int32)
    j = rs.randint(0, n_items, B).astype(np.int32)
    i[: B // 3] = 0                                   # a hot, duplicated positive item
    j[B // 3: B // 3 + B // 8] = 1                    # and a duplicated negative one
    return u, i, j


def run_mf_trajectory(ops, B, d, steps, n_users, n_items, seed):
    dp = ops.padded_dim(d)
    P, Q, w, rs = mf_problem(seed, n_users, n_items, d)
    ref = bpr_ref.Adam([P, Q], LR)
    state = ops.MFState(ops.pad_cols(dev(P), dp), ops.pad_cols(dev(Q), dp), ops.pad_cols(dev(w), dp), ops.pad_cols(dev(w), dp),
                        hyper(ops), B)
    losses = []
    for t in range(steps):
        u, i, j = mf_batch(rs, n_users, n_items, B)
        want = bpr_ref.mf_bpr(ref.params[0], ref.params[1], u, i, j, DECAY, BS)
        got = state.step(ops.LOSS_BPR, dev(u), dev(i), dev(j)).cpu().numpy()
        np.testing.assert_allclose(got, want[:3], rtol=1e-5, err_msg="step %d" % t)
        ref.step(want[3:])
        losses.append(got)
    return state, ref, np.asarray(losses)


@pytest.mark.parametrize("d", [32, 48, 64, 128, 256])
@pytest.mark.parametrize("B", [96, 257, 1024, 4096])
def test_mf_bpr_twenty_step_trajectory(ops, B, d):
    """20 steps on the small-batch path (atomics, positives combined per chunk) against the float64 restatement; d = 48
    runs at 64 with zero columns, which must stay zero."""
    steps = 20
    state, ref, _ = run_mf_trajectory(ops, B, d, steps, 5000, 700, 1000 + B + d)
    for name, mine, theirs in (("P", state.P, ref.params[0]), ("Q", state.Q, ref.params[1])):
        m = mine.cpu().numpy()
        assert not m[:, d:].any(), name
        diff = np.abs(m[:, :d] - theirs)
        assert diff.max() <= 2e-3 * LR * steps and diff.mean() <= 1e-4 * LR * steps, (name, diff.max(), diff.mean())
    for name, mine, theirs in (("mP", state.mP, ref.m[0]), ("mQ", state.mQ, ref.m[1]), ("vP", state.vP, ref.v[0]),
                               ("vQ", state.vQ, ref.v[1])):
        np.testing.assert_allclose(mine.cpu().numpy()[:, :d], theirs, rtol=2e-4, atol=2e-6 * np.abs(theirs).max(), err_msg=name)
    assert float(state.gP.abs().max()) == 0.0 and float(state.gQ.abs().max()) == 0.0     # scratch consumed
    assert int(state.tP.sum()) == 0 and int(state.tQ.sum()) == 0


@pytest.mark.parametrize("B", [16384, 65536])
def test_mf_bpr_staged_path_trajectory_and_determinism(ops, B):
    """Above 8192 triples: staged gradient rows, references sorted by row -- on the restatement for 20 steps (hot rows
    included).  Every row has one owner that sums its references in sorted order; only rows referenced more than a
    16-reference chunk's worth add atomically (train_kernels.hip, k_seg_reduce).  Without such rows two runs of 20 steps
    give the same bits."""
    steps, d = 20, 64
    a, ref, _ = run_mf_trajectory(ops, B, d, steps, 70000, 3000, 7 + B)
    for name, mine, theirs in (("P", a.P, ref.params[0]), ("Q", a.Q, ref.params[1])):
        diff = np.abs(mine.cpu().numpy() - theirs)
        assert diff.max() <= 2e-3 * LR * steps and diff.mean() <= 1e-4 * LR * steps, (name, diff.max(), diff.mean())
    n_users, n_items = 70000, 400000
    P, Q, w, rs = mf_problem(11 + B, n_users, n_items, d)
    batches = []
    for _ in range(steps):
        u = rs.choice(n_users, B, replace=False).astype(np.int32)
        ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)      # every item row once per batch
        batches.append((dev(u), dev(ij[:B]), dev(ij[B:])))
    runs = []
    for _ in range(2):
        st = ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B)
        losses = [st.step(ops.LOSS_BPR, *b).clone() for b in batches]
        runs.append((st, torch.stack(losses)))
    (sa, la), (sb, lb) = runs
    assert torch.equal(la, lb)
    for name in ("P", "Q", "mP", "vP", "mQ", "vQ"):
        assert torch.equal(getattr(sa, name), getattr(sb, name)), name


# ----------------------------------------------------------------------------- LightGCN
def lgcn_graph(seed, n_users, n_items, n_inter, asym):
    rs = np.random.RandomState(seed)
    R = sp.coo_matrix((np.ones(n_inter), (rs.randint(0, n_users, n_inter), rs.zipf(1.3, n_inter) % n_items)),
                      shape=(n_users, n_items)).tocsr()
    R.data[:] = 1.0
    R = (R + sp.csr_matrix((np.ones(n_users), (np.arange(n_users), rs.randint(0, n_items, n_users))), shape=R.shape)).tocsr()
    R = (R + sp.csr_matrix((np.ones(n_items), (rs.randint(0, n_users, n_items), np.arange(n_items))), shape=R.shape)).tocsr()
    R.data[:] = 1.0
    A = sp.bmat([[None, R], [R.T, None]]).tocsr()
    deg = np.asarray(A.sum(1)).ravel()
    if asym:
        M = sp.diags(1.0 / deg).dot(A)                                # D^-1 A: --adj_type norm / mean
    else:
        M = sp.diags(deg ** -0.5).dot(A).dot(sp.diags(deg ** -0.5))   # --adj_type pre
    M = M.tocsr().astype(np.float32)
    M.sort_indices()
    return M, rs


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("n_layers", [1, 2, 3])
@pytest.mark.parametrize("asym", [False, True])
def test_lightgcn_bpr_steps(ops, asym, n_layers, d):
    """Five steps (symmetric `pre` adjacency: macr_lgcn_train_step's A in both places; D^-1 A: the transposed CSR of
    macr_lgcn_train_step_t) against the restatement, then MACR_STEP_LOSS_ONLY: the step's losses, nothing written."""
    n_users, n_items, B, steps = 500, 300, 512, 5
    M, rs = lgcn_graph(7 * n_layers + d + asym, n_users, n_items, 4000, asym)
    Mt = M.T.tocsr()
    Mt.sort_indices()
    T0 = (rs.standard_normal((n_users + n_items, d)) * 0.1).astype(np.float32)
    w0 = (rs.standard_normal(d) * 0.3).astype(np.float32)
    adj = ops.CSR.from_scipy(M, "cuda")
    adj_t = ops.CSR.from_scipy(Mt, "cuda") if asym else None
    state = ops.LGCNState(dev(T0), n_users, n_items, dev(w0), dev(w0), adj, n_layers, hyper(ops), B, adj_t=adj_t)
    M64, Mt64 = M.astype(np.float64), Mt.astype(np.float64)
    ref = bpr_ref.Adam([T0], LR)
    for t in range(steps):
        u, i, j = mf_batch(rs, n_users, n_items, B)
        want = bpr_ref.lgcn_bpr(M64, ref.params[0], n_users, n_layers, u, i, j, DECAY, BS, At=Mt64)
        got = state.step(ops.LOSS_BPR_LGCN, dev(u), dev(i), dev(j)).cpu().numpy()
        np.testing.assert_allclose(got, want[:3], rtol=2e-5, err_msg="step %d" % t)
        ref.step([want[3]])
    diff = np.abs(state.T.cpu().numpy() - ref.params[0])
    assert diff.max() <= 2e-3 * LR * steps and diff.mean() <= 1e-4 * LR * steps, (diff.max(), diff.mean())
    np.testing.assert_allclose(state.mT.cpu().numpy(), ref.m[0], rtol=5e-4, atol=5e-6 * np.abs(ref.m[0]).max())
    # loss-only pass: the losses of the batch as of now, T / w / w_user / every slot / adam_pow bitwise unchanged
    u, i, j = mf_batch(rs, n_users, n_items, B)
    want = bpr_ref.lgcn_bpr(M64, state.T.cpu().numpy().astype(np.float64), n_users, n_layers, u, i, j, DECAY, BS, At=Mt64)
    before = {n: getattr(state, n).clone() for n in ("T", "w", "wu", "mT", "vT", "mw", "vw", "mwu", "vwu", "adam_pow")}
    got = state.step(ops.LOSS_BPR_LGCN, dev(u), dev(i), dev(j), loss_only=True).cpu().numpy()
    np.testing.assert_allclose(got, want[:3], rtol=2e-5)
    for n, v in before.items():
        assert torch.equal(getattr(state, n), v), n


# ----------------------------------------------------------------------------- row-sharded entry points, deferral
@pytest.mark.parametrize("B,d", [(1000, 64), (300, 256), (20000, 128)])
def test_row_shard_world1_bpr_equals_unsharded_step(ops, B, d):
    from macr_amd import sharded_train
    n_users, n_items = 30000, 900
    P, Q, w, rs = mf_problem(B + d, n_users, n_items, d)
    shard = sharded_train.RowShardedMF(dev(P), dev(Q), dev(w), dev(w),
                                       sharded_train.HipBackend(ops.LOSS_BPR, d, hyper(ops), torch.device("cuda")), rank=0, world=1)
    plain = ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B)
    for t in range(3):
        u, i, j = mf_batch(rs, n_users, n_items, B)
        a = shard.step(dev(u), dev(i), dev(j)).cpu().numpy()
        b = plain.step(ops.LOSS_BPR, dev(u), dev(i), dev(j)).cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=1e-6, err_msg="step %d" % t)
    for name, x, y in (("P", shard.P, plain.P), ("Q", shard.Q, plain.Q), ("mP", shard.mP, plain.mP), ("mQ", shard.mQ, plain.mQ)):
        y = y.cpu().numpy()
        np.testing.assert_allclose(x.cpu().numpy(), y, rtol=1e-5, atol=1e-6 * np.abs(y).max(), err_msg=name)
    assert np.array_equal(shard.w.cpu().numpy(), w) and np.array_equal(shard.wu.cpu().numpy(), w)


def test_defer_is_ignored_for_bpr(ops):
    """defer=True asks for the deferred Adam pass, which only the (B,B) losses have: a BPR step completes in the call, the
    same call as without it (every row once per batch, so that no gradient row is summed by atomics in a varying order)"""
    d, B, n_users, n_items = 64, 700, 2000, 4000
    P, Q, w, rs = mf_problem(3, n_users, n_items, d)
    a = ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B)
    b = ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B)
    for t in range(4):
        u = rs.choice(n_users, B, replace=False).astype(np.int32)
        i, j = rs.choice(n_items, 2 * B, replace=False).astype(np.int32).reshape(2, B)
        la = a.step(ops.LOSS_BPR, dev(u), dev(i), dev(j), defer=True)
        assert a.pending_B == 0
        lb = b.step(ops.LOSS_BPR, dev(u), dev(i), dev(j))
        assert torch.equal(la, lb)
    for name in ("P", "Q", "mP", "vP", "mQ", "vQ"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ----------------------------------------------------------------------------- models: session shim, memory
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=256, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


def test_session_shim_bpr_matches_fast_path(ops):
    from macr_amd.mf import BPRMF, Session
    cfg = dict(n_users=900, n_items=300)
    a, b = BPRMF(_mf_args(), cfg, seed=7), BPRMF(_mf_args(), cfg, seed=7)
    sess = Session(a)
    rs = np.random.RandomState(0)
    for _ in range(3):
        u = rs.choice(900, 256, replace=False).tolist(); i = rs.randint(0, 300, 256).tolist(); j = rs.randint(0, 300, 256).tolist()
        _, loss, mf, reg = sess.run([a.opt, a.loss, a.mf_loss, a.reg_loss], feed_dict={a.users: u, a.pos_items: i, a.neg_items: j})
        direct = b.train_step(ops.LOSS_BPR, b.to_device_batch(u, i, j)).cpu().numpy()
        np.testing.assert_allclose([loss, mf, reg], direct, rtol=1e-6)
    # (equal up to the order in which the small-batch path's atomics add a duplicated item's gradient rows)
    for x, y in ((a.user_embedding, b.user_embedding), (a.item_embedding, b.item_embedding)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-7)
    with pytest.raises(NotImplementedError):
        sess.run(a.opt_two, {a.users: u, a.pos_items: i, a.neg_items: j})
    # a checkpoint of the run carries the BPR optimizer; a fresh model takes it back
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    assert "opt%d.adam_pow" % ops.LOSS_BPR in sd
    c = BPRMF(_mf_args(), cfg, seed=9)
    c.load_state_dict(sd)
    for name in ("mP", "vP", "mQ", "vQ", "adam_pow"):
        assert torch.equal(getattr(c.opt_state(ops.LOSS_BPR), name), getattr(a.opt_state(ops.LOSS_BPR), name)), name


def _lgcn(ops, n_users=400, n_items=250):
    from macr_amd.lightgcn import LightGCN
    M, _ = lgcn_graph(5, n_users, n_items, 3000, False)
    args = types.SimpleNamespace(adj_type="pre", alg_type="lightgcn", lr=1e-3, embed_size=64, batch_size=256,
                                 layer_size="[64,64]", regs="[1e-5]", verbose=0, Ks="[20]", alpha=1e-2, beta=1e-3,
                                 dataset="synthetic", node_dropout_flag=0)
    return LightGCN(dict(n_users=n_users, n_items=n_items, norm_adj=M), args, seed=3)


def test_lightgcn_session_shim_bpr(ops):
    from macr_amd.mf import Session
    a, b = _lgcn(ops), _lgcn(ops)
    sess = Session(a)
    rs = np.random.RandomState(1)
    u = rs.choice(400, 256, replace=False).tolist(); i = rs.randint(0, 250, 256).tolist(); j = rs.randint(0, 250, 256).tolist()
    _, loss, mf, emb, reg = sess.run([a.opt, a.loss, a.mf_loss, a.emb_loss, a.reg_loss],
                                     feed_dict={a.users: u, a.pos_items: i, a.neg_items: j})
    direct = b.train_step(ops.LOSS_BPR_LGCN, b.to_device_batch(u, i, j)).cpu().numpy()
    np.testing.assert_allclose([loss, mf, emb], direct, rtol=1e-6)
    assert float(np.asarray(reg).ravel()[0]) == 0.0                    # tf.constant(0.) (:411)
    torch.testing.assert_close(a.T, b.T, rtol=1e-5, atol=1e-7)


def test_bpr_state_exists_only_once_used(ops):
    """Constructing the models and training normalbce / bce allocates what it did before BPR existed; the BPR optimizer
    (table-sized Adam slots) appears with the first BPR step."""
    from macr_amd.mf import BPRMF
    torch.cuda.synchronize()
    cfg = dict(n_users=20000, n_items=3000)
    base = torch.cuda.memory_allocated()
    m = BPRMF(_mf_args(), cfg, seed=1)
    rs = np.random.RandomState(2)
    batch = m.to_device_batch(rs.choice(20000, 256, replace=False), rs.randint(0, 3000, 256), rs.randint(0, 3000, 256))
    m.train_step(ops.LOSS_NORMALBCE, batch)
    torch.cuda.synchronize()
    assert ops.LOSS_BPR not in m._opt and len(m._opt) == 3
    used = torch.cuda.memory_allocated() - base
    table = (20000 + 3000) * 64 * 4                 # P and Q
    # the parameters + three optimizers of m, v and gradient scratch for each table (3 tables each), small buffers aside
    assert used < (1 + 3 * 3 + 1) * table, used
    m.train_step(ops.LOSS_BPR, batch)
    torch.cuda.synchronize()
    assert ops.LOSS_BPR in m._opt and torch.cuda.memory_allocated() - base - used >= 3 * table
    g = _lgcn(ops)
    assert ops.LOSS_BPR_LGCN not in g._opt and len(g._opt) == 2
    g.train_step(ops.LOSS_NORMALBCE, g.to_device_batch(rs.choice(400, 64), rs.randint(0, 250, 64), rs.randint(0, 250, 64)))
    assert ops.LOSS_BPR_LGCN not in g._opt
    g.train_step(ops.LOSS_BPR_LGCN, g.to_device_batch(rs.choice(400, 64), rs.randint(0, 250, 64), rs.randint(0, 250, 64)))
    assert ops.LOSS_BPR_LGCN in g._opt and g._opt[ops.LOSS_BPR_LGCN].T is g.T


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _run(cmd, cwd, ok=True):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    if ok:
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out


def _tiny(tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    return str(tmp_path / "data") + "/"


def _train_losses(out):
    vals = [float(l.split("train==[")[1].split("=")[0]) for l in out.splitlines() if "train==[" in l]
    assert vals and all(np.isfinite(vals)), out
    return vals


@pytest.mark.parametrize("sampler", ["reference", "device"])
def test_mf_cli_train_normal(tmp_path, sampler):
    data = _tiny(tmp_path)
    out = _run([os.path.join(REPO, "macr_mf", "train.py"), "--data_path", data, "--dataset", "tiny_data", "--batch_size", "16",
                "--cuda", "0", "--saveID", "n", "--log_interval", "1", "--lr", "0.01", "--epoch", "6", "--train", "normal",
                "--test", "normal", "--Ks", "[5]", "--sampler", sampler, "--save_flag", "0"], str(tmp_path)).stdout
    vals = _train_losses(out)
    assert len(vals) == 6 and vals[-1] < vals[0], out
    assert out.count("recall=[") == 6, out
    bad = _run([os.path.join(REPO, "macr_mf", "train.py"), "--data_path", data, "--dataset", "tiny_data", "--batch_size", "16",
                "--cuda", "0", "--saveID", "r", "--log_interval", "1", "--epoch", "2", "--train", "normal", "--test", "rubi",
                "--Ks", "[5]", "--save_flag", "0"], str(tmp_path), ok=False)
    assert bad.returncode != 0 and "--test rubi needs a branch loss" in bad.stderr, bad.stderr[-2000:]


@pytest.mark.parametrize("sampler", ["reference", "device"])
def test_lightgcn_cli_default_loss_is_bpr(tmp_path, sampler):
    data = _tiny(tmp_path)
    out = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py"), "--data_path", data, "--dataset", "tiny_data", "--verbose", "1",
                "--layer_size", "[64,64]", "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0", "--epoch", "7",
                "--log_interval", "2", "--weights_path", str(tmp_path) + "/", "--saveID", "b", "--sampler", sampler],
               str(tmp_path)).stdout
    vals = _train_losses(out)
    assert len(vals) >= 3 and vals[-1] < vals[0], out
    tests = [l for l in out.splitlines() if "test==[" in l]
    assert len(tests) == 3 and all("recall=[" in l for l in tests), out
