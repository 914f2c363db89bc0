"""The DEFAULT (atomic, non-deterministic) LightGCN step under `--loss bce` / `--loss bceboth` on the GPU (-m gpu): the path
the README's MACR-LightGCN command trains on and bench.py times, against the float64 restatement of tests/lgcn_both_ref.py
(pinned to the reference's graph code by tests/test_lgcn_both_cpu.py, which also shows the fp32 oracle inside a tenth of the
bounds below).

1. Twenty steps per case on lgcn_graph(500 x 300), B = 512, users with replacement and positives by Zipf, at 0 to 5 layers
   (0: k_scale_copy both ways; 1: the layers run dense; >= 2: row-sparse layers and the fused optimizer; 4: the first layer that
   overwrites a layer buffer pair) and d = 32 .. 256; subsets on the row-normalised adjacency with its transpose, with
   dense_layers=True, without a plan and at B = 300 (the plain (B,B) launch).  Every number is one the suite already holds the
   same step code to:
     each step's losses   rtol 1e-5                                   (test_lgcn_train_step_matches_oracle)
     final T, w, wu       max |diff| <= 2e-3 lr steps, mean <= 1e-4 lr steps    (test_twenty_step_trajectory)
     final slots          rtol 2e-4, atol 2e-6 max |want|             (test_mf_twenty_step_trajectory_stays_on_the_oracle)
     adam_pow             its initial value times (0.9^20, 0.999^20), rtol 1e-6
     bce                  w, wu bitwise their initial values, their four slots all zero
     after every step and after a closing loss-only step: every scratch region of the workspace zero
     (spmm_cases.lgcn_scratch_regions); the closing step leaves all state bit-identical and gives the restatement's losses
2. One workspace through twelve calls that alternate the route (default / dense_layers), loss-only and the kind (all five) on
   the SMALL hub graph: per-call losses, final tensors at the same bounds, scratch regions zero after every call."""
import functools

import numpy as np
import pytest
import torch

import bpr_ref
import lgcn_both_ref as lb
import lgcn_branch_ref
import spmm_cases as sc
from test_gpu_lgcn_deterministic import KINDS, LOSS_RTOL

pytestmark = pytest.mark.gpu

STATE_NAMES = ("T", "w", "wu") + lb.SLOTS + ("adam_pow",)
BRANCH_SLOTS = ("mw", "vw", "mwu", "vwu")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a writable copy: the problems' arrays are read-only)


# (asym, d, L, route, B); route: default / dense (dense_layers=True) / noplan
CASES = [(False, d, L, "default", 512) for d in (32, 64, 128, 256) for L in range(6)]
CASES += [(True, d, L, "default", 512) for d in (32, 128) for L in (1, 2, 4)]
CASES += [(False, d, L, "dense", 512) for d in (64, 256) for L in (2, 4)]
CASES += [(False, 64, L, "noplan", 512) for L in (2, 4)]
CASES += [(False, 64, L, "default", 300) for L in (0, 2, 5)]
IDS = ["%s-d%d-L%d-%s-B%d" % ("rownorm" if a else "sym", d, L, r, B) for a, d, L, r, B in CASES]


@functools.lru_cache(maxsize=None)
def device_graph(asym, L, d, plan):
    from macr_amd import ops
    pr = lb.problem(asym, L, d, 512)                                 # (the graph does not depend on B)
    env = {} if plan else None
    return sc.device_csr(ops, pr["A"], env), (sc.device_csr(ops, pr["At"], env) if asym else None)


def dirt(regions):
    """{region: non-zero entries} in one trip to the host (NaN counts)"""
    names = sorted(regions)
    counts = torch.stack([(regions[n] != 0).sum() for n in names]).cpu().tolist()
    return {n: c for n, c in zip(names, counts) if c}


def report(record_property, what, ratios):
    for k, v in sorted(ratios.items()):
        record_property(k, v)
    print("%s: diff / bound %s" % (what, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))


def final_ratios(state, want, names):
    """worst diff / bound of the final tensors (lgcn_both_ref.used; the slots' ' rtol' shares are informative only)"""
    ratios = {}
    for name in names:
        ratios.update({k: v for k, v in lb.used(getattr(state, name).cpu().numpy(), want[name], name).items() if not k.endswith(" rtol")})
    return ratios


@pytest.mark.parametrize("kind", ["bce", "bceboth"])
@pytest.mark.parametrize("asym,d,L,route,B", CASES, ids=IDS)
def test_default_step_stays_on_the_float64_trajectory(ops, asym, d, L, route, B, kind, record_property):
    pr, ref = lb.problem(asym, L, d, B), lb.reference(kind, asym, L, d, B)
    adj, adj_t = device_graph(asym, L, d, route != "noplan")
    assert (adj.plan_host is None) == (route == "noplan")
    state = ops.LGCNState(dev(pr["T"]), lb.N_USERS, lb.N_ITEMS, dev(pr["w"]), dev(pr["wu"]), adj, L,
                          ops.make_hyper(lb.LR, lb.DECAY, lb.ALPHA, lb.BETA, lb.BS), B, adj_t=adj_t)
    pow0 = state.adam_pow.cpu().numpy().astype(np.float64)
    regions = sc.lgcn_scratch_regions(ops, state)
    assert {"dE", "cnt", "emb_acc", "sbr"} <= set(regions) and ("arrivals" in regions) == (route != "noplan")
    k, dense = getattr(ops, KINDS[kind]), route == "dense"
    worst = 0.0
    for t, (u, i, j) in enumerate(pr["batches"][:lb.STEPS]):
        got = state.step(k, dev(u), dev(i), dev(j), dense_layers=dense).cpu().numpy().astype(np.float64)
        worst = max(worst, float((np.abs(got - ref["losses"][t]) / np.abs(ref["losses"][t])).max() / 1e-5))
        np.testing.assert_allclose(got, ref["losses"][t], rtol=1e-5, err_msg="step %d" % t)
        assert not dirt(regions), "step %d left %r" % (t, dirt(regions))
    ratios = {"losses": worst}
    ratios.update(final_ratios(state, ref, ("T", "w", "wu", "mT", "vT") + (BRANCH_SLOTS if kind == "bceboth" else ())))
    want_pow = pow0 * np.array([0.9 ** lb.STEPS, 0.999 ** lb.STEPS])
    ratios["adam_pow"] = float((np.abs(state.adam_pow.cpu().numpy() - want_pow) / want_pow).max() / 1e-6)
    report(record_property, "%s %s" % (kind, IDS[CASES.index((asym, d, L, route, B))]), ratios)
    assert max(ratios.values()) <= 1.0, ratios
    if kind == "bce":                                   # neither branch vector is in bce's graph: nothing may touch them
        assert np.array_equal(state.w.cpu().numpy().view(np.uint32), pr["w"].view(np.uint32))
        assert np.array_equal(state.wu.cpu().numpy().view(np.uint32), pr["wu"].view(np.uint32))
        for name in BRANCH_SLOTS:
            assert not getattr(state, name).any(), name
    # a closing loss-only step: the losses of a fresh batch as of now, nothing written, nothing left behind
    before = {n: getattr(state, n).clone() for n in STATE_NAMES}
    u, i, j = pr["batches"][lb.STEPS]
    got = state.step(k, dev(u), dev(i), dev(j), loss_only=True, dense_layers=dense).cpu().numpy()
    np.testing.assert_allclose(got, ref["losses"][lb.STEPS], rtol=1e-5, err_msg="loss-only step")
    for n, v in before.items():
        assert torch.equal(getattr(state, n).view(torch.int32), v.view(torch.int32)), "the loss-only step wrote %s" % n
    assert not dirt(regions), "the loss-only step left %r" % dirt(regions)


# ----------------------------------------------------------------------------- one workspace, mixed calls
# (kind, dense_layers, loss_only): every kind on both routes or loss-only, every change of route with and without a loss-only
# call in between, the ego kind (which uses sbr) before and after kinds that do not
SEQUENCE = (("bceboth", False, False), ("bce", True, False), ("bce1", False, True), ("bce2", False, False), ("bpr", True, False),
            ("bceboth", True, True), ("bce1", True, False), ("bce", False, False), ("bce2", True, True), ("bpr", False, False),
            ("bce2", True, False), ("bceboth", False, False))


def test_one_workspace_through_mixed_calls(ops, record_property):
    """include/macr_hip.h: the workspace's flags and counters are 'zero between steps: every step leaves them that way', while
    MACR_STEP_LOSS_ONLY and MACR_STEP_DENSE_LAYERS are per call.  d = 64, three layers, SMALL under D^-1/2 A D^-1/2 (hub rows of
    two groups: arrival counters and hub finishers in play), B = 256, spmm_cases.hub_batch.  Reference: ONE bpr_ref.Adam over
    [T, w, w_user] stepped with the gradient of the restatement the call's kind names; a vector the kind does not train is
    left out of that step (Adam.step zips), as the C oracle leaves it out."""
    d, L, B = 64, 3, 256
    n_users, n_items = sc.SMALL_SHAPE
    A = sc.sym_norm(sc.small())
    A64 = A.astype(np.float64)
    rs = np.random.RandomState(41)
    T0 = (rs.standard_normal((n_users + n_items, d)) * 0.1).astype(np.float32)
    w0, wu0 = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    adj = sc.device_csr(ops, A, {})
    assert max(sc.groups_per_row(sc.decode_plan(adj.plan_host)).values()) >= 2
    state = ops.LGCNState(dev(T0), n_users, n_items, dev(w0), dev(wu0), adj, L, ops.make_hyper(lb.LR, lb.DECAY, lb.ALPHA, lb.BETA, lb.BS), B)
    pow0 = state.adam_pow.cpu().numpy().astype(np.float64)
    regions = sc.lgcn_scratch_regions(ops, state)
    assert regions["arrivals"].numel() >= 64 + 2
    ref = bpr_ref.Adam([T0, w0, wu0], lb.LR)

    def restated(kind, u, i, j):
        """-> (the three losses, the gradients of the vectors the kind trains, in the order T, w, w_user)"""
        T, w, wu = ref.params
        if kind in ("bce", "bceboth"):
            out = lb.lgcn_both(A64, T, w, wu, n_users, L, u, i, j, lb.ALPHA, lb.BETA, lb.DECAY, lb.BS, both=kind == "bceboth", At=A64)
            return out[:3], list(out[3:]) if kind == "bceboth" else [out[3]]
        if kind == "bpr":
            out = bpr_ref.lgcn_bpr(A64, T, n_users, L, u, i, j, lb.DECAY, lb.BS, At=A64)
            return out[:3], [out[3]]
        out = lgcn_branch_ref.lgcn_item_branch(A64, T, w, n_users, L, u, i, j, lb.ALPHA, lb.DECAY, lb.BS, ego=kind == "bce2", At=A64)
        return out[:3], [out[3], out[4]]

    steps, ratios = 0, {}
    for c, (kind, dense, loss_only) in enumerate(SEQUENCE):
        what = "call %d (%s%s%s)" % (c, kind, ", dense layers" if dense else "", ", loss only" if loss_only else "")
        u, i, j = sc.hub_batch(rs, n_users, n_items, B)
        want, grads = restated(kind, u, i, j)
        before = {n: getattr(state, n).clone() for n in STATE_NAMES} if loss_only else None
        got = state.step(getattr(ops, KINDS[kind]), dev(u), dev(i), dev(j), loss_only=loss_only, dense_layers=dense).cpu().numpy()
        rel = float((np.abs(got.astype(np.float64) - want) / np.abs(want)).max() / LOSS_RTOL[kind])
        ratios["losses " + kind] = max(ratios.get("losses " + kind, 0.0), rel)
        print("%s: got %r want %r" % (what, got.tolist(), [float(x) for x in want]))
        np.testing.assert_allclose(got, want, rtol=LOSS_RTOL[kind], err_msg=what)
        assert not dirt(regions), "%s left %r" % (what, dirt(regions))
        if loss_only:
            for n, v in before.items():
                assert torch.equal(getattr(state, n).view(torch.int32), v.view(torch.int32)), "%s wrote %s" % (what, n)
        else:
            ref.step(grads)
            steps += 1
    assert steps == 9 and ref.t == 9
    want = dict(T=ref.params[0], w=ref.params[1], wu=ref.params[2], mT=ref.m[0], vT=ref.v[0], mw=ref.m[1], vw=ref.v[1],
                mwu=ref.m[2], vwu=ref.v[2])
    for name in ("T", "w", "wu") + lb.SLOTS:
        ratios.update({k: v for k, v in lb.used(getattr(state, name).cpu().numpy(), want[name], name, steps=steps).items()
                       if not k.endswith(" rtol")})
    want_pow = pow0 * np.array([0.9 ** steps, 0.999 ** steps])
    ratios["adam_pow"] = float((np.abs(state.adam_pow.cpu().numpy() - want_pow) / want_pow).max() / 1e-6)
    report(record_property, "mixed calls", ratios)
    assert max(ratios.values()) <= 1.0, ratios
