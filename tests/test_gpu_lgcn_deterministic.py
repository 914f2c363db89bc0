"""The bit-reproducible LightGCN step on the GPU (-m gpu): LGCNState(deterministic=True) / MACR_STEP_DETERMINISTIC on
macr_lgcn_train_step(_t) / MACR_DETERMINISTIC=1.

Every shape is the smallest that reaches a place where the order of a sum could leak; the hot runs are written by hand over a
random batch, then permuted, with a fresh batch per step (chunks of k_seg_reduce: 16 references, 8 at d = 32):

    S_hub      spmm_cases.small() under sym_norm, default plan (hub items of one and two groups), d 64, 2 layers, B 300:
               i[:150] = 0, j[150:225] = 1, u[:150] = 3 -- runs of ten chunks in both halves of the table; the hub rows are
               batch rows, so a hub finisher runs the fused epilogue; by default the small-batch atomic route
    S_chunk64  lgcn_graph(500 x 300), plan built under MACR_SPMM_CHUNK=64, d 32, 3 layers, B 96: item 0 48 times, chunks of 8
    S_asym     spmm_cases.small() under row_norm (a transposed plan of its own), d 128, 2 layers, B 257: item 0 130 times
    S_dense1   lgcn_graph(500 x 300), d 256, ONE layer (the step then runs its layers dense), B 300, hot runs as S_hub:
    S_dense2   ... and two layers with dense_layers=True: k_reg_scatter's replacement and k_adam_dense
    S_staged   lgcn_graph(9001 x 1201), d 64, 2 layers, B 8448: item 0 1000 times -- by default already the staged route
    S_stream   S_hub with the plan built under MACR_SPMM_STREAM=1; bceboth only
    S_noplan   lgcn_graph(500 x 300) without a plan (one wave per row, no hub pieces), d 64, 2 layers, B 96; bceboth only

1. repeatability: three fresh deterministic states, six steps on the same batches, then a loss-only step: the losses of every
   step, T, w, wu, the six slots, adam_pow and the loss-only losses equal BIT FOR BIT.  Whether two default-mode states
   differed on the same batches is put on record, not asserted.
2. accuracy: the same trajectories against the CPU restatements the existing tests use (oracle.lgcn_train_step for bce /
   bceboth, tests/bpr_ref.py for bpr, tests/lgcn_branch_ref.py for bce1 / bce2) at those tests' tolerances.
3. hygiene: one step from equal states, deterministic against default; the per-row counts zero after every deterministic
   step; the kernels each mode launches.
4. the model under MACR_DETERMINISTIC=1 and pairs of runs of the LightGCN CLI: bit-identical checkpoints."""
import functools
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
from helpers import GOLD, REPO
from spmm_cases import SMALL_SHAPE, device_csr, hub_batch, hub_graph, lgcn_counts, plan_env, row_norm, small, sym_norm  # noqa: F401
from test_gpu_lgcn_branch import lgcn_graph

pytestmark = pytest.mark.gpu

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-4, 1e-2, 1e-3, 1024
STEPS = 6
STATE_NAMES = ("T", "w", "wu", "mT", "vT", "mw", "vw", "mwu", "vwu", "adam_pow")
KINDS = {"bce": "LOSS_NORMALBCE", "bceboth": "LOSS_RUBIBCEBOTH", "bpr": "LOSS_BPR_LGCN", "bce1": "LOSS_RUBIBCE", "bce2": "LOSS_RUBIBCE_EGO"}
BXB = ("bceboth", "bce1", "bce2")
HUB_RUNS = (("i", 0, 150, 0), ("j", 150, 225, 1), ("u", 0, 150, 3))

# name -> (graph, plan knobs, d, layers, dense_layers, B, hot runs)
SHAPES = {
    "S_hub": ("small_sym", {}, 64, 2, False, 300, HUB_RUNS),
    "S_chunk64": ("g500", {"MACR_SPMM_CHUNK": "64"}, 32, 3, False, 96, (("i", 0, 48, 0),)),
    "S_asym": ("small_row", {}, 128, 2, False, 257, (("i", 0, 130, 0),)),
    "S_dense1": ("g500", {}, 256, 1, False, 300, HUB_RUNS),
    "S_dense2": ("g500", {}, 256, 2, True, 300, HUB_RUNS),
    "S_staged": ("g9001", {}, 64, 2, False, 8448, (("i", 0, 1000, 0),)),
    "S_stream": ("small_sym", {"MACR_SPMM_STREAM": "1"}, 64, 2, False, 300, HUB_RUNS),
    "S_noplan": ("g500", None, 64, 2, False, 96, (("i", 0, 48, 0),)),
}
CASES = [(s, k) for s in SHAPES for k in KINDS if s not in ("S_stream", "S_noplan") or k == "bceboth"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a writable copy: the problems' arrays are read-only)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (A, A^T or None, n_users, n_items)"""
    if name == "small_sym":
        return sym_norm(small()), None, SMALL_SHAPE[0], SMALL_SHAPE[1]
    if name == "small_row":
        A, At = row_norm(small())
        return A, At, SMALL_SHAPE[0], SMALL_SHAPE[1]
    if name == "g500":
        return lgcn_graph(21, 500, 300, 4000, False)[0], None, 500, 300
    assert name == "g9001"
    return lgcn_graph(22, 9001, 1201, 40000, False)[0], None, 9001, 1201


@functools.lru_cache(maxsize=None)
def problem(shape):
    """table, branch vectors and STEPS + 1 batches (the last one for the loss-only step), the shape's hot runs in every one"""
    gname, _, d, _, _, B, hot = SHAPES[shape]
    _, _, n_users, n_items = graph(gname)
    rs = np.random.RandomState(B + d + len(shape))
    T = (rs.standard_normal((n_users + n_items, d)) * 0.1).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    batches = []
    for _ in range(STEPS + 1):
        b = dict(u=rs.choice(n_users, B, replace=B > n_users).astype(np.int32), i=rs.randint(0, n_items, B).astype(np.int32),
                 j=rs.randint(0, n_items, B).astype(np.int32))
        for name, lo, hi, row in hot:
            b[name][lo:hi] = row
        o = rs.permutation(B)                                       # the hot references spread over the batch's blocks
        batches.append(tuple(b[k][o] for k in ("u", "i", "j")))
    for a in (T, w, wu) + tuple(x for b in batches for x in b):
        a.setflags(write=False)
    return T, w, wu, tuple(batches)


@functools.lru_cache(maxsize=None)
def device_batches(shape):
    return tuple(tuple(dev(x) for x in b) for b in problem(shape)[3])


@functools.lru_cache(maxsize=None)
def device_graph(shape):
    """the adjacency (and its transpose) on the device with plans built under the shape's knobs"""
    from macr_amd import ops
    gname, env = SHAPES[shape][:2]
    A, At, _, _ = graph(gname)
    adj = device_csr(ops, A, env)
    return adj, (device_csr(ops, At, env) if At is not None else None)


def fresh(ops, shape, deterministic):
    gname, _, d, L, _, B, _ = SHAPES[shape]
    _, _, n_users, n_items = graph(gname)
    T, w, wu, _ = problem(shape)
    adj, adj_t = device_graph(shape)
    st = ops.LGCNState(dev(T), n_users, n_items, dev(w), dev(wu), adj, L, ops.make_hyper(LR, DECAY, ALPHA, BETA, BS), B, adj_t=adj_t,
                       deterministic=deterministic)
    assert st.deterministic == deterministic
    return st


def snapshot(state):
    return {n: getattr(state, n).clone() for n in STATE_NAMES}


def run(ops, shape, kind, deterministic, first=None):
    """STEPS steps and a loss-only step from the problem's initial arrays -> (losses (STEPS + 1, 3), final state); first: dict
    that receives mT, mw, mwu after the first step"""
    k = getattr(ops, KINDS[kind])
    dense = SHAPES[shape][4]
    state = fresh(ops, shape, deterministic)
    batches = device_batches(shape)
    losses = []
    for t, (u, i, j) in enumerate(batches[:STEPS]):
        losses.append(state.step(k, u, i, j, dense_layers=dense).clone())
        if deterministic:
            assert not lgcn_counts(ops, state).any(), "%s %s step %d: reference counts left behind" % (shape, kind, t)
        if first is not None and t == 0:
            first.update({n: getattr(state, n).clone() for n in ("mT", "mw", "mwu")})
    before = snapshot(state)
    u, i, j = batches[STEPS]
    losses.append(state.step(k, u, i, j, loss_only=True, dense_layers=dense).clone())
    for n, v in before.items():
        assert torch.equal(getattr(state, n), v), "loss-only step wrote %s" % n
    if deterministic:
        assert not lgcn_counts(ops, state).any(), "%s %s loss-only: reference counts left behind" % (shape, kind)
    return torch.stack(losses), before


def bits_equal(a, b):
    """same shape, same bits (NaNs of equal payload included)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- 1. repeatability
@pytest.mark.parametrize("shape,kind", CASES)
def test_deterministic_runs_are_bit_identical(ops, shape, kind, record_property):
    runs = [run(ops, shape, kind, True) for _ in range(3)]
    l0, s0 = runs[0]
    assert bool(torch.isfinite(l0).all()), l0
    for k, (l, s) in enumerate(runs[1:], 1):
        assert bits_equal(l, l0), ("losses", k, l, l0)
        for n in STATE_NAMES:
            assert bits_equal(s[n], s0[n]), (n, k, float((s[n] - s0[n]).abs().max()))
    # the default step on the same batches: on record, not asserted (its atomics' order is the hardware's)
    (la, sa), (lb, sb) = run(ops, shape, kind, False), run(ops, shape, kind, False)
    differed = sorted(n for n in STATE_NAMES if not bits_equal(sa[n], sb[n])) + ([] if bits_equal(la, lb) else ["losses"])
    record_property("default_mode_bits_differed", bool(differed))
    record_property("default_mode_differing", ",".join(differed))
    print("%s %s: default mode differed in %s" % (shape, kind, differed or "nothing"))


# ----------------------------------------------------------------------------- 2. accuracy
@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    """the CPU trajectory of a problem, once: losses per step (the loss-only step last), (dT, dw, dwu) of the first step, final
    T, w, wu"""
    gname, _, d, L, _, B, _ = SHAPES[shape]
    A, At, n_users, n_items = graph(gname)
    T0, w0, wu0, batches = problem(shape)
    losses, g1 = [], None
    if kind in ("bce", "bceboth"):
        To, wo, wuo = T0.copy(), w0.copy(), wu0.copy()
        st = oracle.AdamState([T0.shape, (d,), (d,)])
        tr = None if At is None else (At.indptr, At.indices, At.data)
        okind = getattr(oracle, KINDS[kind])
        for u, i, j in batches[:STEPS]:
            losses.append(np.asarray(oracle.lgcn_train_step(okind, n_users, n_items, L, A.indptr, A.indices, A.data, u, i, j, To, wo, wuo,
                                                            st, LR, DECAY, ALPHA, BETA, BS, transposed=tr)).copy())
            if g1 is None:
                g1 = [st.m[0] / 0.1, st.m[1] / 0.1 if kind == "bceboth" else None, st.m[2] / 0.1 if kind == "bceboth" else None]
        final = (To.copy(), wo.copy(), wuo.copy())
        # the loss-only step: one more oracle step on copies (its losses are those of the parameters before its update)
        u, i, j = batches[STEPS]
        st2 = oracle.AdamState([T0.shape, (d,), (d,)])
        losses.append(np.asarray(oracle.lgcn_train_step(okind, n_users, n_items, L, A.indptr, A.indices, A.data, u, i, j, To.copy(),
                                                        wo.copy(), wuo.copy(), st2, LR, DECAY, ALPHA, BETA, BS, transposed=tr)).copy())
        return losses, g1, final
    A64 = A.astype(np.float64)
    At64 = None if At is None else At.astype(np.float64)
    if kind == "bpr":
        ref = bpr_ref.Adam([T0], LR)
        step = lambda u, i, j: bpr_ref.lgcn_bpr(A64, ref.params[0], n_users, L, u, i, j, DECAY, BS, At=At64)
    else:
        ref = bpr_ref.Adam([T0, w0], LR)
        step = lambda u, i, j: lgcn_branch_ref.lgcn_item_branch(A64, ref.params[0], ref.params[1], n_users, L, u, i, j, ALPHA, DECAY,
                                                                BS, ego=kind == "bce2", At=At64)
    for u, i, j in batches[:STEPS]:
        out = step(u, i, j)
        ref.step(list(out[3:]))
        losses.append(np.asarray(out[:3]))
        if g1 is None:
            g1 = [ref.m[0].copy() / 0.1, (ref.m[1].copy() / 0.1 if kind != "bpr" else None), None]
    losses.append(np.asarray(step(*batches[STEPS])[:3]))
    return losses, g1, (ref.params[0], ref.params[1] if kind != "bpr" else w0, wu0)


# what the existing tests of each kind ask: losses (spmm_cases.run_train_case: 1e-5, bpr 2e-5; test_gpu_lgcn_branch: 5e-5) and
# the first step's gradient through mT / 0.1 (rtol, atol as a fraction of the largest entry)
LOSS_RTOL = {"bce": 1e-5, "bceboth": 1e-5, "bpr": 2e-5, "bce1": 5e-5, "bce2": 5e-5}
GRAD_TOL = {"bce": (5e-4, 2e-6), "bceboth": (5e-4, 2e-6), "bpr": (5e-4, 5e-6), "bce1": (5e-4, 2e-6), "bce2": (5e-4, 2e-6)}


@pytest.mark.parametrize("shape,kind", CASES)
def test_deterministic_trajectory_matches_the_cpu_restatement(ops, shape, kind):
    want_losses, g1, (Tw, ww, wuw) = reference(shape, kind)
    first = {}
    losses, s = run(ops, shape, kind, True, first=first)
    losses = losses.cpu().numpy()
    for t in range(STEPS + 1):
        print("%s %s step %d: got %r want %r" % (shape, kind, t, losses[t].tolist(), np.asarray(want_losses[t]).tolist()))
        np.testing.assert_allclose(losses[t], want_losses[t], rtol=LOSS_RTOL[kind], err_msg="step %d" % t)
    rtol, afrac = GRAD_TOL[kind]
    for name, got, want in (("dT", first["mT"], g1[0]), ("dw", first["mw"], g1[1]), ("dwu", first["mwu"], g1[2])):
        got = got.cpu().numpy() / 0.1
        if want is None:                                   # a vector this loss does not train
            assert not got.any(), name
            continue
        print("%s %s %s: max |err| %.3g of max %.3g" % (shape, kind, name, np.abs(got - want).max(), np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=rtol, atol=afrac * np.abs(want).max(), err_msg=name)
    for name, want in (("T", Tw), ("w", ww), ("wu", wuw)):
        diff = np.abs(s[name].cpu().numpy() - want)
        print("%s %s %s: max %.3g mean %.3g (bounds %.3g, %.3g)" % (shape, kind, name, diff.max(), diff.mean(), 2e-3 * LR * STEPS,
                                                                   1e-4 * LR * STEPS))
        assert diff.max() <= 2e-3 * LR * STEPS and diff.mean() <= 1e-4 * LR * STEPS, (name, diff.max(), diff.mean())


# ----------------------------------------------------------------------------- 3. hygiene
NEW_KERNELS = {"reg_rows", "emb_fold"}


@pytest.mark.parametrize("shape,kind", CASES)
def test_one_deterministic_step_agrees_with_the_default_step(ops, shape, kind):
    k = getattr(ops, KINDS[kind])
    dense = SHAPES[shape][4]
    det, plain = fresh(ops, shape, True), fresh(ops, shape, False)
    u, i, j = device_batches(shape)[0]
    ops.timing_begin()
    a = det.step(k, u, i, j, dense_layers=dense).cpu().numpy()
    det_kernels = {n for n, _ in ops.timing_end(256)}
    ops.timing_begin()
    b = plain.step(k, u, i, j, dense_layers=dense).cpu().numpy()
    plain_kernels = {n for n, _ in ops.timing_end(256)}
    print("%s %s: deterministic %s\n  default %s" % (shape, kind, sorted(det_kernels), sorted(plain_kernels)))
    assert {"seg_reduce", "seg_fold"} | NEW_KERNELS <= det_kernels and "reg_scatter" not in det_kernels, det_kernels
    assert ("branch_fold" in det_kernels) == (kind in BXB), det_kernels
    assert not (NEW_KERNELS | {"seg_fold", "branch_fold"}) & plain_kernels, plain_kernels
    fused = SHAPES[shape][3] > 1 and not dense
    assert ("adam_dense" in det_kernels) == (not fused) and ("lgcn_finalize" in det_kernels) == fused, det_kernels
    np.testing.assert_allclose(a, b, rtol=1e-6)
    for name in ("T", "mT"):
        x, y = getattr(det, name).cpu().numpy(), getattr(plain, name).cpu().numpy()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6 * np.abs(y).max(), err_msg=name)
    assert not lgcn_counts(ops, det).any()
    assert torch.equal(det.adam_pow, plain.adam_pow)


# ----------------------------------------------------------------------------- 4. model and CLI
def _lgcn(**kw):
    from macr_amd.lightgcn import LightGCN
    M = graph("g500")[0]
    args = types.SimpleNamespace(adj_type="pre", alg_type="lightgcn", lr=1e-3, embed_size=64, batch_size=300,
                                 layer_size="[64,64]", regs="[1e-4]", verbose=0, Ks="[20]", alpha=1e-2, beta=1e-3,
                                 dataset="synthetic", node_dropout_flag=0)
    return LightGCN(dict(n_users=500, n_items=300, norm_adj=M), args, seed=3, **kw)


@pytest.mark.parametrize("loss", list(KINDS))
def test_models_under_the_variable_train_bit_identically(ops, loss, monkeypatch):
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")
    a, b = _lgcn(), _lgcn()
    monkeypatch.delenv("MACR_DETERMINISTIC")
    off, kw = _lgcn(), _lgcn(deterministic=True)               # without the variable: off; the keyword alone turns it on
    assert a.deterministic and b.deterministic and kw.deterministic and not off.deterministic
    kind = a.kind_of(loss)
    for u, i, j in problem("S_dense1")[3][:4]:                  # hot-row batches on 500 x 300
        for m in (a, b, kw):
            m.train_step(kind, m.to_device_batch(u.tolist(), i.tolist(), j.tolist()))
    for m in (a, b, kw):                                        # every state, the on-demand ones included
        assert kind in m._opt and all(st.deterministic for st in m._opt.values())
    assert not any(st.deterministic for st in off._opt.values())
    sa, sb, sk = a.state_dict(), b.state_dict(), kw.state_dict()
    assert sorted(sa) == sorted(sb) == sorted(sk) and "opt%d.adam_pow" % kind in sa
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert bits_equal(sa[k], sb[k]) and bits_equal(sa[k], sk[k]), k
        else:
            assert sa[k] == sb[k] == sk[k], k
    assert not torch.equal(sa["T"], off.T)                      # (it trained)


def _cli_run(tmp, loss, test):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp / "data" / "tiny_data")
    env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_DETERMINISTIC="1")
    cmd = [sys.executable, os.path.join(REPO, "macr_lightgcn", "LightGCN.py"), "--data_path", str(tmp / "data") + "/", "--dataset",
           "tiny_data", "--verbose", "1", "--layer_size", "[64,64]", "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0",
           "--epoch", "4", "--log_interval", "2", "--weights_path", str(tmp) + "/", "--saveID", "det", "--loss", loss, "--test", test,
           "--c", "0.5", "--save_flag", "1", "--seed", "5"]
    out = subprocess.run(cmd, cwd=str(tmp), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ckpts = {}
    for root, _, files in os.walk(str(tmp)):
        for f in files:
            if f.startswith("weights_") and f.endswith(".pt"):
                ckpts[f] = torch.load(os.path.join(root, f), map_location="cpu")
    return out.stdout, ckpts


@pytest.mark.parametrize("loss,test", [("bceboth", "rubiboth"), ("bce2", "rubi2")])
def test_lightgcn_cli_runs_are_bit_identical(tmp_path, loss, test):
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    (out_a, ck_a), (out_b, ck_b) = _cli_run(tmp_path / "a", loss, test), _cli_run(tmp_path / "b", loss, test)
    assert sorted(ck_a) == sorted(ck_b) == ["weights_det-2.pt", "weights_det-4.pt"], (sorted(ck_a), sorted(ck_b))
    for f in ck_a:
        assert sorted(ck_a[f]) == sorted(ck_b[f])
        for k, v in ck_a[f].items():
            if torch.is_tensor(v):
                assert bits_equal(v, ck_b[f][k]), (f, k)
            else:
                assert v == ck_b[f][k], (f, k)
    assert not torch.equal(ck_a["weights_det-2.pt"]["T"], ck_a["weights_det-4.pt"]["T"])
    train = lambda out: [l.split("train==[")[1].split("]")[0] for l in out.splitlines() if "train==[" in l]
    ta, tb = train(out_a), train(out_b)
    assert len(ta) == 2 and ta == tb, (ta, tb)
    tests = lambda out: [l for l in out.splitlines() if l.startswith("c:")]
    print("CLI %s: test lines identical: %s" % (loss, tests(out_a) == tests(out_b)))       # (evaluator metrics: outside the contract)
