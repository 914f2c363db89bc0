"""MF two-branch BPR loss on the HIP path (-m gpu): `--train rubi` (MACR_LOSS_RUBIBPR, macr_mf/model.py:124-156).  One step
against the reference's graph code (G13), multi-step trajectories against the float64 restatement of tests/rubi_bpr_ref.py,
the deferred, lazy and staged forms of the step, the fp32 overflow the reference has too, the model and the CLI."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bpr_ref
import rubi_bpr_ref
from helpers import GOLD, REPO, golden_npz_parts

pytestmark = pytest.mark.gpu

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 1024
INPUTS = ("P", "Q", "w", "wu", "u", "i", "j")
_MF_NAMES = ("P", "Q", "w", "wu", "mP", "vP", "mQ", "vQ", "mw", "vw", "mwu", "vwu")


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


def g13():
    with np.load(os.path.join(GOLD, "G13_mf_rubi_bpr.npz")) as z:
        return {k: z[k] for k in z.files}


def hyper(ops):
    return ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)


# ----------------------------------------------------------------------------- one step against the reference's graph
@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_rubi_bpr_step_matches_reference_graph(ops, tag):
    """a / b / c: G10's problems; d: logits in [-71.7, 57.7] -- every cell finite in fp32 though far from 0.  (These batches
    are below 4096 triples: one row per lane, no shared logarithm; test_rubi_bpr_window_edge_at_row_pairs is the row-pair
    form's window test.)"""
    G = g13()
    if tag == "d":
        g = lambda k: G["mf_d/in/%s" % k]
    else:
        G10 = golden_npz_parts("G10_model_steps")
        g = lambda k: G10["mf_%s/%s" % (tag, k)]
    w0, wu0 = g("w").reshape(-1), g("wu").reshape(-1)
    state = ops.MFState(dev(g("P")), dev(g("Q")), dev(w0), dev(wu0), hyper(ops), len(g("u")))
    got = state.step(ops.LOSS_RUBIBPR, dev(g("u"), torch.int32), dev(g("i"), torch.int32), dev(g("j"), torch.int32)).cpu().numpy()
    print("case %s: loss %r" % (tag, got.tolist()))
    for dt in ("f32", "f64"):
        want = [float(G["mf_%s/rubi_bpr/%s/%s" % (tag, dt, k)]) for k in ("loss", "mf_loss", "reg_loss")]
        np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=dt)
    pre = "mf_%s/rubi_bpr/f64/" % tag
    close_grad(state.mP.cpu().numpy() / 0.1, G[pre + "dP"], "dP", 2e-4)
    close_grad(state.mQ.cpu().numpy() / 0.1, G[pre + "dQ"], "dQ", 2e-4)
    close_grad(state.mw.cpu().numpy() / 0.1, G[pre + "dw"].reshape(-1), "dw", 2e-4)
    assert not np.array_equal(state.w.cpu().numpy(), w0)                    # w is trained (opt_two, :64-66)
    assert np.array_equal(state.wu.cpu().numpy(), wu0)                      # no user branch: w_user bitwise untouched
    assert not state.mwu.cpu().numpy().any() and not state.vwu.cpu().numpy().any()


# ----------------------------------------------------------------------------- the row-pair form's window
@pytest.mark.parametrize("B", [4096, 4200])
def test_rubi_bpr_window_edge_at_row_pairs(ops, B):
    """From 4096 triples on a lane holds four rows and the (B,B) kernel takes ONE logarithm for the cells of two rows -- which
    overflows when Z1 + Z2 < -88 although each cell is finite in the reference, so such waves must take one logarithm per
    cell.  mf_problem(21, 6000, 900, 32, B, 1.6): every cell above -88 (min Z about -70), row pairs of a lane down to
    about -136; B = 4096: full tiles, B = 4200: partial ones.  Two steps against the float64 restatement: a finite loss
    within rtol 1e-5, gradients within the bounds of the G13 test."""
    P, Q, w, wu, u, i, j = rubi_bpr_ref.mf_problem(21, 6000, 900, 32, B, 1.6)
    w, wu = w.reshape(-1), wu.reshape(-1)
    r = np.arange(B)
    first = r[((r % 256) // 64) % 2 == 0]                  # rows q*64 + lane, q even, of a 256-row block; their pair: + 64
    first = first[first + 64 < B]
    ref = bpr_ref.Adam([P, Q, w], LR)
    state = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), hyper(ops), B)
    rs = np.random.RandomState(5)
    for t in range(2):
        Z = rubi_bpr_ref.z_matrix(ref.params[0], ref.params[1], ref.params[2], u, i, j)
        pair_min = float((Z[first] + Z[first + 64]).min())
        print("B %d step %d: min Z %.1f, min Z1 + Z2 of a lane's row pair %.1f" % (B, t, Z.min(), pair_min))
        assert -85.0 < Z.min() < -44.0 and pair_min < -100.0          # the case is what the docstring says it is
        del Z
        want = rubi_bpr_ref.mf_rubi_bpr(ref.params[0], ref.params[1], ref.params[2], u, i, j, ALPHA, DECAY, BS)
        got = state.step(ops.LOSS_RUBIBPR, dev(u, torch.int32), dev(i, torch.int32), dev(j, torch.int32)).cpu().numpy()
        print("step %d: got %r want %r" % (t, got.tolist(), list(want[:3])))
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want[:3], rtol=1e-5, err_msg="step %d" % t)
        if t == 0:
            close_grad(state.mP.cpu().numpy() / 0.1, want[3], "dP", 2e-4)
            close_grad(state.mQ.cpu().numpy() / 0.1, want[4], "dQ", 2e-4)
            close_grad(state.mw.cpu().numpy() / 0.1, want[5], "dw", 2e-4)
        ref.step(want[3:])
        o = rs.permutation(B)                              # the same triples (the same logits) on other lanes and row pairs
        u, i, j = u[o], i[o], j[o]
    assert np.isfinite(state.P.cpu().numpy()).all() and np.isfinite(state.Q.cpu().numpy()).all()


# ----------------------------------------------------------------------------- trajectories
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


def run_trajectory(ops, B, d, steps, n_users, n_items, seed, ref_device=None):
    dp = ops.padded_dim(d)
    P, Q, w, rs = mf_problem(seed, n_users, n_items, d)
    ref = bpr_ref.Adam([P, Q, w], LR)
    state = ops.MFState(ops.pad_cols(dev(P), dp), ops.pad_cols(dev(Q), dp), ops.pad_cols(dev(w), dp), ops.pad_cols(dev(w), dp),
                        hyper(ops), B)
    for t in range(steps):
        u, i, j = mf_batch(rs, n_users, n_items, B)
        want = rubi_bpr_ref.mf_rubi_bpr(ref.params[0], ref.params[1], ref.params[2], u, i, j, ALPHA, DECAY, BS, device=ref_device)
        got = state.step(ops.LOSS_RUBIBPR, dev(u), dev(i), dev(j)).cpu().numpy()
        np.testing.assert_allclose(got, want[:3], rtol=1e-5, err_msg="step %d" % t)
        ref.step(want[3:])
    return state, ref, w


def check_against_ref(state, ref, d, steps, w0):
    for name, mine, theirs in (("P", state.P, ref.params[0]), ("Q", state.Q, ref.params[1]), ("w", state.w, ref.params[2])):
        m = mine.cpu().numpy().reshape(-1, mine.shape[-1])
        assert not m[:, d:].any(), name                                   # padded columns stay zero
        diff = np.abs(m[:, :d] - theirs.reshape(-1, d))
        assert diff.max() <= 2e-3 * LR * steps and diff.mean() <= 1e-4 * LR * steps, (name, diff.max(), diff.mean())
    for name, mine, theirs in (("mP", state.mP, ref.m[0]), ("mQ", state.mQ, ref.m[1]), ("vP", state.vP, ref.v[0]),
                               ("vQ", state.vQ, ref.v[1]), ("mw", state.mw, ref.m[2]), ("vw", state.vw, ref.v[2])):
        m = mine.cpu().numpy().reshape(-1, mine.shape[-1])[:, :d]
        np.testing.assert_allclose(m, theirs.reshape(-1, d), rtol=2e-4, atol=2e-6 * np.abs(theirs).max(), err_msg=name)
    assert float(state.gP.abs().max()) == 0.0 and float(state.gQ.abs().max()) == 0.0     # scratch consumed
    assert int(state.tP.sum()) == 0 and int(state.tQ.sum()) == 0
    assert np.array_equal(state.wu.cpu().numpy()[:d], w0)                 # (w_user started as a copy of w) never touched
    assert not state.mwu.cpu().numpy().any() and not state.vwu.cpu().numpy().any()


@pytest.mark.parametrize("d", [32, 48, 64, 128, 256])
@pytest.mark.parametrize("B", [96, 257, 1024, 4096])
def test_rubi_bpr_twenty_step_trajectory(ops, B, d):
    """20 steps on the small-batch path against the float64 restatement: one row per lane below 4096 triples, row pairs at
    4096; partial tiles at 96 and 257; d = 48 runs at 64 with zero columns, which must stay zero."""
    steps = 20
    state, ref, w0 = run_trajectory(ops, B, d, steps, 5000, 700, 2000 + B + d)
    check_against_ref(state, ref, d, steps, w0)


# ----------------------------------------------------------------------------- deferred and lazy forms
@pytest.mark.parametrize("B,d,n_users,n_items,sort", [(96, 64, 300, 50, False), (257, 64, 300, 50, True),
                                                      (1024, 64, 13485, 744, True), (64, 32, 100, 40, True),
                                                      (128, 128, 500, 300, False), (64, 256, 100, 40, True),
                                                      (4096, 64, 3000, 900, True)])
def test_rubi_bpr_deferred_equals_complete_steps(ops, B, d, n_users, n_items, sort):
    """MACR_STEP_DEFER / MACR_STEP_PENDING: the dense Adam pass of step t rides in the (B,B) launch of step t+1.  Per-step
    losses equal those of complete steps; after flush() so does the state, up to the order of the float atomics."""
    P, Q, w, rs = mf_problem(B + d + 1, n_users, n_items, d)
    wu = (rs.standard_normal(d) * 0.3).astype(np.float32)
    lazy = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), hyper(ops), B)
    eager = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), hyper(ops), B)
    ref = bpr_ref.Adam([P, Q, w], LR)
    for t in range(5):
        u, i, j = mf_batch(rs, n_users, n_items, B)
        if t == 2:
            i[: B // 2] = 3                         # a different hot item
        if sort:
            o = np.argsort(i, kind="stable")
            u, i, j = u[o], i[o], j[o]
        want = rubi_bpr_ref.mf_rubi_bpr(ref.params[0], ref.params[1], ref.params[2], u, i, j, ALPHA, DECAY, BS)
        ref.step(want[3:])
        got = lazy.step(ops.LOSS_RUBIBPR, dev(u), dev(i), dev(j), defer=True).cpu().numpy()
        plain = eager.step(ops.LOSS_RUBIBPR, dev(u), dev(i), dev(j)).cpu().numpy()
        np.testing.assert_allclose(got, want[:3], rtol=1e-5, atol=0)
        np.testing.assert_allclose(got, plain, rtol=2e-6, atol=0)
        assert lazy.pending_B == B and eager.pending_B == 0
    lazy.flush()
    assert lazy.pending_B == 0
    for name in _MF_NAMES:
        a, b = getattr(lazy, name).cpu().numpy(), getattr(eager, name).cpu().numpy()
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-7 + 1e-5 * np.abs(b).max(), err_msg=name)
    np.testing.assert_allclose(lazy.P.cpu().numpy(), ref.params[0], rtol=0, atol=0.02 * LR * 5)
    np.testing.assert_allclose(lazy.Q.cpu().numpy(), ref.params[1], rtol=0, atol=0.02 * LR * 5)
    assert float(lazy.gP.abs().max()) == 0.0 and float(lazy.gQ.abs().max()) == 0.0
    assert int(lazy.tP.sum()) == 0 and int(lazy.tQ.sum()) == 0
    np.testing.assert_array_equal(lazy.adam_pow.cpu().numpy(), eager.adam_pow.cpu().numpy())
    assert np.array_equal(lazy.wu.cpu().numpy(), wu) and not lazy.mwu.cpu().numpy().any()


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_rubi_bpr_lazy_sequence_equals_the_dense_sequence_bit_for_bit(ops, d):
    """Batches without a repeated row and with at most eight backward blocks: every atomic add of a step lands on a zero, so a
    deferred sequence is reproducible bit for bit -- and the lazy Adam form (periods 2, 3, 7) must reproduce the dense form:
    every step's losses, and after a flush every table and slot (what tests/test_gpu_lazy_adam.py requires of rubibce)."""
    n_users, n_items, B, steps = 2000, 1500, 128, 26
    P, Q, w, rs = mf_problem(9 + d, n_users, n_items, d)
    states = [ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B, lazy_period=k) for k in (1, 2, 3, 7)]
    for step in range(steps):
        u = rs.choice(n_users, B, replace=False).astype(np.int32)
        ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)
        b = [dev(a) for a in (u, ij[:B], ij[B:])]
        losses = [s.step(ops.LOSS_RUBIBPR, *b, defer=True).clone() for s in states]
        assert states[1]._seq_lazy is not None and states[0]._seq_lazy is None
        for l in losses[1:]:
            assert torch.equal(l, losses[0]), (step, l, losses[0])
        if step in (9, steps - 1):
            for s in states:
                s.flush()
            for s in states[1:]:
                for name in _MF_NAMES:
                    assert torch.equal(getattr(s, name), getattr(states[0], name)), (step, name)
                assert int(s.tP.abs().sum()) == 0 and int(s.tQ.abs().sum()) == 0 and float(s.gP.abs().max()) == 0.0
                st, sp, sq = s._lazy_bufs
                assert int(sp.min()) == step + 1 and int(sq.max()) == step + 1
    # a lazy sequence ended by a step that completes in its call
    u = rs.choice(n_users, B, replace=False).astype(np.int32)
    ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)
    b = [dev(a) for a in (u, ij[:B], ij[B:])]
    for defer in (True, False):
        out = [s.step(ops.LOSS_RUBIBPR, *b, defer=defer).clone() for s in states[:2]]
        assert torch.equal(out[0], out[1])
    for name in _MF_NAMES:
        assert torch.equal(getattr(states[1], name), getattr(states[0], name)), name


# ----------------------------------------------------------------------------- staged path (B > 8192)
@pytest.mark.parametrize("B", [16384, 1 << 17])
def test_rubi_bpr_staged_path(ops, B, monkeypatch):
    """Above 8192 triples: gradient rows staged, references sorted by row, no atomics on the tables, the Adam pass summing the
    staged rows itself (indexed).  Two steps against the restatement (hot rows included); one step from the same state twice
    gives the same losses and table gradients bit for bit (every row has one owner summing in list order; w's gradient meets
    in a few partial rows by atomics, as for rubibce: equal up to their order); MACR_SEG_UNFUSED=1 (the segment reduce writes
    every gradient row) agrees with the indexed pass."""
    monkeypatch.delenv("MACR_SEG_UNFUSED", raising=False)
    steps, d = 2, 64
    n_users, n_items = (70000, 3000) if B == 16384 else (200000, 20000)
    state, ref, w0 = run_trajectory(ops, B, d, steps, n_users, n_items, 7 + B, ref_device="cuda")     # (float64, in slabs)
    check_against_ref(state, ref, d, steps, w0)
    n_items = 4 * B
    P, Q, w, rs = mf_problem(11 + B, n_users, n_items, d)
    batches = []
    for _ in range(steps):
        u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
        ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)      # every item row once per batch
        batches.append((dev(u), dev(ij[:B]), dev(ij[B:])))
    runs = []
    for unfused in (False, False, True):
        if unfused:
            monkeypatch.setenv("MACR_SEG_UNFUSED", "1")
        st = ops.MFState(dev(P), dev(Q), dev(w), dev(w), hyper(ops), B)
        ops.timing_begin()
        first = st.step(ops.LOSS_RUBIBPR, *batches[0]).clone()
        names = {n for n, _ in ops.timing_end(64)}
        assert ("adam_indexed" in names) == (not unfused) and ("seg_reduce" in names) == unfused, names
        g1 = (st.mP.clone(), st.mQ.clone(), st.mw.clone())
        second = st.step(ops.LOSS_RUBIBPR, *batches[1]).clone()
        runs.append((st, first, g1, second))
    (sa, la, ga, la2), (sb, lb, gb, lb2), (sc, lc, gc, lc2) = runs
    assert torch.equal(la, lb) and torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    torch.testing.assert_close(ga[2], gb[2], rtol=1e-5, atol=1e-9)
    torch.testing.assert_close(la2, lb2, rtol=2e-6, atol=0)
    torch.testing.assert_close(la, lc, rtol=2e-6, atol=0)
    torch.testing.assert_close(la2, lc2, rtol=2e-6, atol=0)
    for other in (sb, sc):
        for name in _MF_NAMES:
            a, b = getattr(sa, name).cpu().numpy(), getattr(other, name).cpu().numpy()
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-7 + 1e-5 * np.abs(b).max(), err_msg=name)
        assert float(other.gP.abs().max()) == 0.0 and float(other.gQ.abs().max()) == 0.0
        assert int(other.tP.sum()) == 0 and int(other.tQ.sum()) == 0


# ----------------------------------------------------------------------------- overflow
def test_rubi_bpr_overflow_is_arithmetic_only(ops):
    """The reference computes log(sigmoid(Z)) literally: below about -88 fp32 sigmoid is 0, the loss +inf, the gradient NaN
    (mf_problem(14, 90, 50, 32, 96, 2.0): min Z = -100.7; the reference's float32 run returns inf).  Nothing is clamped here
    either: the step returns MACR_OK with a non-finite loss, and the next step on a fresh state works."""
    P, Q, w, wu, u, i, j = rubi_bpr_ref.mf_problem(14, 90, 50, 32, 96, 2.0)
    args = (dev(u, torch.int32), dev(i, torch.int32), dev(j, torch.int32))
    for defer in (False, True):
        state = ops.MFState(dev(P), dev(Q), dev(w.reshape(-1)), dev(wu.reshape(-1)), hyper(ops), len(u))
        got = state.step(ops.LOSS_RUBIBPR, *args, defer=defer).cpu().numpy()       # (raises unless the call returned MACR_OK)
        print("overflow, defer=%s: %r" % (defer, got.tolist()))
        assert not np.isfinite(got[0]) and not np.isfinite(got[1]) and np.isfinite(got[2])
        state.flush()
        torch.cuda.synchronize()
    P, Q, w, wu, u, i, j = rubi_bpr_ref.mf_problem(14, 90, 50, 32, 96, 1.7)
    fresh = ops.MFState(dev(P), dev(Q), dev(w.reshape(-1)), dev(wu.reshape(-1)), hyper(ops), len(u))
    got = fresh.step(ops.LOSS_RUBIBPR, dev(u, torch.int32), dev(i, torch.int32), dev(j, torch.int32)).cpu().numpy()
    np.testing.assert_allclose(got[0], float(g13()["mf_d/rubi_bpr/f64/loss"]), rtol=1e-5)
    assert np.isfinite(fresh.P.cpu().numpy()).all() and np.isfinite(fresh.Q.cpu().numpy()).all()


# ----------------------------------------------------------------------------- model
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=256, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


def test_model_trains_rubi_and_checkpoints_its_optimizer(ops):
    from macr_amd.mf import BPRMF, ShardedBPRMF, Session
    cfg = dict(n_users=900, n_items=300)
    a = BPRMF(_mf_args(), cfg, seed=7)
    kind = a.kind_of("rubi")
    assert kind == ops.LOSS_RUBIBPR and kind not in a._opt and len(a._opt) == 3       # created on demand
    direct = ops.MFState(a.user_embedding.clone(), a.item_embedding.clone(), a.w.clone(), a.w_user.clone(),
                         ops.make_hyper(1e-3, 1e-5, 1e-2, 1e-3, 256), 256)             # (the hyper-parameters of _mf_args)
    rs = np.random.RandomState(0)
    for _ in range(3):
        u = rs.choice(900, 256, replace=False); i = rs.choice(300, 256, replace=False); j = rs.choice(300, 256, replace=False)
        batch = a.to_device_batch(u.tolist(), i.tolist(), j.tolist())
        got = a.train_step(kind, batch).cpu().numpy()
        want = direct.step(kind, batch[0], batch[1], batch[2]).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-6)
    assert kind in a._opt and a.opt_state(kind).P is a.user_embedding
    for x, y in ((a.user_embedding, direct.P), (a.item_embedding, direct.Q), (a.w, direct.w)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-7)
    assert torch.equal(a.w_user, direct.wu)
    # the session shim has no fetch of this kind: opt_two stays outside it
    with pytest.raises(NotImplementedError):
        Session(a).run(a.opt_two, {a.users: u.tolist(), a.pos_items: i.tolist(), a.neg_items: j.tolist()})
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    assert "opt6.adam_pow" in sd and "opt6.mw" in sd
    c = BPRMF(_mf_args(), cfg, seed=9)
    c.load_state_dict(sd)
    for name in ("mP", "vP", "mQ", "vQ", "mw", "vw", "adam_pow"):
        assert torch.equal(getattr(c.opt_state(kind), name), getattr(a.opt_state(kind), name)), name
    with pytest.raises(NotImplementedError):
        ShardedBPRMF.kind_of(ShardedBPRMF.__new__(ShardedBPRMF), "rubi")


# ----------------------------------------------------------------------------- CLI
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _cli(script, tmp_path, *extra):
    return _run([os.path.join(REPO, "macr_mf", script), "--data_path", os.path.join(REPO, "data") + "/", "--dataset", "addressa",
                 "--train", "rubi", "--epoch", "2", "--log_interval", "1", "--cuda", "0", "--saveID", "rubi", "--save_flag", "0",
                 "--alpha", "1e-2"] + list(extra), str(tmp_path))


def _metrics(line):
    """the numbers of a report line (losses and metrics), all finite"""
    assert "nan" not in line.lower() and "inf" not in line.lower(), line
    vals = [float(x) for x in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", line.split("]: ", 1)[1])]
    assert len(vals) >= 11 and all(np.isfinite(vals)), line          # train==[3], recall, precision, hit, ndcg [2 each]
    return vals


@pytest.mark.parametrize("sampler", ["reference", "device"])
def test_mf_cli_train_rubi(tmp_path, sampler):
    out = _cli("train.py", tmp_path, "--test", "rubi", "--c", "40", "--sampler", sampler)
    lines = [l for l in out.splitlines() if l.startswith("c:40.00")]
    assert len(lines) == 2 and all("recall=[" in l and "train==[" in l for l in lines), out
    for l in lines:
        _metrics(l)


def test_mf_cli_train_rubi_test_normal_and_tune(tmp_path):
    out = _cli("train.py", tmp_path, "--test", "normal")
    lines = [l for l in out.splitlines() if l.startswith("Epoch ") and "recall=[" in l]
    assert len(lines) == 2, out
    for l in lines:
        _metrics(l)
    out = _cli("tune.py", tmp_path, "--test", "rubi", "--start", "20", "--end", "40", "--step", "3")
    for c in (20.0, 30.0, 40.0):
        lines = [l for l in out.splitlines() if l.startswith("c:%.2f" % c)]
        assert len(lines) == 2, out
        for l in lines:
            _metrics(l)
