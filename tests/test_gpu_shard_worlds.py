"""The row-sharded MF step at 2 .. 16 ranks in ONE process (-m gpu): W threads, one GPU context, the production
RowShardedMF.step / step_split on the HIP backend, the three collectives through tests/shard_loopback.py (proved exact on the
CPU by tests/test_shard_loopback_cpu.py).  Every case is the smallest shape that reaches its edge of the macr_shard_* device
code away from rank 0 of a world of 1:

    B300   W3  d64  range        eight 64-row blocks, rank 2 holds blocks 5..7 wholly above B: its slice is EMPTY (n = 0) while
                                 k_bxb still runs on padding; contiguous shards (lo > 0, stride 1); per-pair kinds at W > 1
    B100   W8  d32  interleaved  5 user rows: ranks 5..7 own NO user row; four row blocks for eight ranks (rb0 == rb1: no launch);
                                 ~20 references per user row: the long-run path (k_seg_sum into gP); stride 8
    B64    W8  d32  interleaved  5 user and 6 item rows: ranks 6, 7 own no row at all (per-pair loss: nothing to update)
    B1500  W5  d128 range        24 blocks over 5 ranks: uneven slices
    B4096  W3 / W16  d64         the 4-row (B,B) form, `full`, 16 blocks of 256 positions: 5/5/6 blocks, one block each
    B4352  W3  d64  range        17 blocks of 256
    B257   W2  d256 range
    B777   W3  d64  range, MACR_SEG_UNFUSED=1   k_seg_reduce on a contiguous shard with lo > 0
    B100   W8  d32  5 user rows, MACR_SEG_UNFUSED=1, dense and lazy: k_seg_reduce flags the item rows of a rank without user rows
    B100   W8  d128 split        fewer row blocks than ranks: slices of 12 / 13 positions that start at no block boundary
    lazy   B777 W3 d64, both layouts, K = 2 / 3, five steps (shards of 301/300/300 and 117/117/116 rows), and B100 W8 with
           5 user rows: the lazy pass on ranks whose item rows sit in segment 0

Reference: oracle.mf_train_step (float32 CPU restatement with double accumulation; BPR: the float64 restatement of
tests/bpr_ref.py), with the tolerances of test_row_shard_entry_points_world1 and tests/shard_worker.py: losses 1e-5 relative
on every rank, the first step's gradient (m / 0.1) rtol 2e-4 + 2e-6 of its largest entry, tables and branch vectors within
0.2 % of the Adam steps taken.

W-invariance.  In the replicated step every exchanged buffer is zero outside one rank's entries, and forward, backward and the
branch gradients are computed in full everywhere -- so it is the world-1 computation bit for bit, EXCEPT where three or more
partial sums meet through atomics in an order the hardware picks (two commute: (0 + a) + b == (0 + b) + a):
  - the apply: rows with more than 128 references (three or more work items of k_seg_sum), and with MACR_SEG_UNFUSED=1 any row
    whose run is cut by a 16-reference chunk boundary (the cut depends on where the run starts in the rank's sorted list);
  - the branch-vector gradients of a branch loss: the backward blocks add into 8 partial rows, three or more blocks per row once
    the batch has more than 16 blocks of 1024 / d positions -- the same from one world-1 run to the next.
A run without either is asserted bit-identical to world 1 over ALL steps (losses, tables, slots, w, w_user).  Otherwise the
first step's losses and the first step's gradient of every row at or under the reference limit are asserted bit-identical
(both are sums in a fixed order; later steps read the hot rows and w), whether w / w_user after the first step were equal is
put on record, and the tolerances cover the rest.  The SPLIT step sums its loss and branch-vector partials over the slices
(tolerance; whether the first step's losses equalled world 1's is put on record), but its first-step gradient rows -- hence P and
Q after the first step, row for row at or under the limit -- are the world-1 rows by construction, and asserted so."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import bpr_ref
import oracle
import shard_loopback

pytestmark = pytest.mark.gpu

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 512
ATOMIC_FREE_REFS = 128          # two work items of k_seg_sum: (0 + a) + b == (0 + b) + a


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a writable copy: the problems' arrays are read-only)


@functools.lru_cache(maxsize=None)
def problem(n_users, n_items, d, B, steps):
    """tables, branch vectors and one fresh batch per step (users by choice, zipf positives: hot rows, uniform negatives)"""
    rs = np.random.RandomState(B + d + n_users)
    P = (rs.standard_normal((n_users, d)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    batches = []
    for _ in range(steps):
        u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
        i = (rs.zipf(1.3, B) % n_items).astype(np.int32)
        j = rs.randint(0, n_items, B).astype(np.int32)
        batches.append((u, i, j))
    for a in (P, Q, w, wu):
        a.setflags(write=False)
    return P, Q, w, wu, batches


@functools.lru_cache(maxsize=None)
def reference(shape, kind_name):
    """the single-process CPU run of a problem, once: losses per step, m of P and Q after the first step, final P, Q, w, w_user"""
    P, Q, w, wu, batches = problem(*shape)
    d = P.shape[1]
    if kind_name == "LOSS_BPR":
        ref = bpr_ref.Adam([P, Q], LR)
        losses, m1 = [], None
        for u, i, j in batches:
            loss, mf, reg, dP, dQ = bpr_ref.mf_bpr(ref.params[0], ref.params[1], u, i, j, DECAY, BS)
            ref.step([dP, dQ])
            losses.append(np.asarray([loss, mf, reg]))
            m1 = m1 or (ref.m[0].copy(), ref.m[1].copy())
        return losses, m1, ref.params[0], ref.params[1], w, wu
    Po, Qo, wo, wuo = P.copy(), Q.copy(), w.copy(), wu.copy()
    st = oracle.AdamState([P.shape, Q.shape, (d,), (d,)])
    losses, m1 = [], None
    for u, i, j in batches:
        losses.append(oracle.mf_train_step(getattr(oracle, kind_name), u, i, j, Po, Qo, wo, wuo, st, LR, DECAY, ALPHA, BETA,
                                           BS).copy())
        m1 = m1 or (st.m[0].copy(), st.m[1].copy())
    return losses, m1, Po, Qo, wo, wuo


def max_refs(shape):
    """(per step: references per user row, per item row) of a problem's batches"""
    P, Q, _, _, batches = problem(*shape)
    return [(np.bincount(u, minlength=P.shape[0]), np.bincount(np.concatenate([i, j]), minlength=Q.shape[0])) for u, i, j in batches]


def run_world(ops, world, shape, kind_name, layout, lazy_period):
    """the problem's steps on `world` ranks -> what every rank saw, and the tables reassembled from the shards"""
    from macr_amd import sharded_train
    P, Q, w, wu, batches = problem(*shape)
    d, kind = P.shape[1], getattr(ops, kind_name)
    device = torch.device("cuda")

    def rank_main(rank, comm):
        hyper = ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)
        model = shard_loopback.LoopbackMF(comm, rank, dev(P), dev(Q), dev(w), dev(wu), sharded_train.HipBackend(kind, d, hyper, device),
                                          layout=layout, lazy_period=lazy_period)
        out = dict(losses=[], w=[], wu=[], wire=[], own_u=model.own_u, own_i=model.own_i)
        for k, (u, i, j) in enumerate(batches):
            last = k == len(batches) - 1
            if last:
                ops.timing_begin()
            out["losses"].append(model.step(dev(u), dev(i), dev(j)).cpu().numpy().copy())
            if last:
                out["kernels"] = {n for n, _ in ops.timing_end(128)}
            out["w"].append(model.w.cpu().numpy())
            out["wu"].append(model.wu.cpu().numpy())
            out["wire"].append(model.wire_rows)
            # the gradient scratch and the row flags are left clean by every step, on every rank
            assert not bool(model.gP.any()) and not bool(model.gQ.any()), "step %d: gradient scratch not zero" % k
            assert int(model.tP.sum()) == 0 and int(model.tQ.sum()) == 0, "step %d: row flags left set" % k
            if k == 0:          # (rows the lazy pass has not visited yet hold m = 0 either way: no flush needed, none provoked)
                out["m1P"], out["m1Q"] = model._mP.cpu(), model._mQ.cpu()
        for name in ("P", "Q", "mP", "vP", "mQ", "vQ"):
            out[name] = getattr(model, name).cpu()            # (flushes what the lazy pass left behind)
        return out

    ranks = shard_loopback.run_ranks(world, rank_main, timeout=120.0)
    n_users, n_items = P.shape[0], Q.shape[0]
    full = {}
    for name in ("P", "mP", "vP", "m1P"):
        full[name] = shard_loopback.reassemble([r[name] for r in ranks], [r["own_u"] for r in ranks], n_users).numpy()
    for name in ("Q", "mQ", "vQ", "m1Q"):
        full[name] = shard_loopback.reassemble([r[name] for r in ranks], [r["own_i"] for r in ranks], n_items).numpy()
    return ranks, full


_world1 = {}


def world1(ops, shape, kind_name, lazy_period, unfused):
    """the same batches through the same entry points on one rank owning everything (computed once per configuration)"""
    key = (shape, kind_name, lazy_period, unfused)
    if key not in _world1:
        _world1[key] = run_world(ops, 1, shape, kind_name, "interleaved", lazy_period)
    return _world1[key]


def case(B, W, d, layout, kind, split, n_users=901, n_items=350, lazy=1, unfused=False):
    steps = 5 if lazy > 1 else 3
    name = "B%d-W%d-d%d-%s-%s-%s" % (B, W, d, layout, kind[5:].lower(), "split" if split else "replicated")
    if n_users < W:
        name += "-%dusers" % n_users
    if n_items < W:
        name += "-%ditems" % n_items
    if lazy > 1:
        name += "-lazy%d" % lazy
    if unfused:
        name += "-unfused"
    return pytest.param((n_users, n_items, d, B, steps), W, layout, kind, split, lazy, unfused, id=name)


BOTH, ITEM, NORMAL, BPR = "LOSS_RUBIBCEBOTH", "LOSS_RUBIBCE", "LOSS_NORMALBCE", "LOSS_BPR"
CASES = (
    [case(300, 3, 64, "range", k, s) for k, s in ((BOTH, True), (BOTH, False), (ITEM, True), (ITEM, False), (NORMAL, False), (BPR, False))] +
    [case(100, 8, 32, "interleaved", k, s, n_users=5, n_items=77) for k, s in ((BOTH, True), (BOTH, False), (NORMAL, False))] +
    [case(64, 8, 32, "interleaved", NORMAL, False, n_users=5, n_items=6)] +
    [case(1500, 5, 128, "range", k, s, n_users=5003, n_items=1201) for k, s in ((ITEM, True), (BPR, False))] +
    [case(4096, W, 64, "interleaved", BOTH, s, n_users=5003, n_items=1201) for W in (3, 16) for s in (True, False)] +
    [case(4352, 3, 64, "range", ITEM, True, n_users=5003, n_items=1201)] +
    [case(257, 2, 256, "range", k, s) for k, s in ((BOTH, True), (NORMAL, False))] +
    [case(777, 3, 64, "range", BOTH, False, unfused=True)] +
    [case(100, 8, 32, "interleaved", BOTH, False, n_users=5, n_items=77, unfused=True, lazy=K) for K in (1, 2)] +
    [case(100, 8, 128, "interleaved", BOTH, True)] +
    [case(777, 3, 64, lay, BOTH, s, lazy=K) for lay in ("interleaved", "range") for K in (2, 3) for s in (True, False)] +
    [case(100, 8, 32, "interleaved", BOTH, s, n_users=5, n_items=77, lazy=2) for s in (True, False)])


@pytest.mark.parametrize("shape,world,layout,kind_name,split,lazy,unfused", CASES)
def test_sharded_step_in_process_world(ops, record_property, monkeypatch, shape, world, layout, kind_name, split, lazy, unfused):
    n_users, n_items, d, B, steps = shape
    pair = kind_name in (NORMAL, BPR)
    monkeypatch.setenv("MACR_SHARD_SPLIT", "1" if split else "0")
    monkeypatch.delenv("MACR_SHARD_ROUTE_TORCH", raising=False)
    if unfused:
        monkeypatch.setenv("MACR_SEG_UNFUSED", "1")
    else:
        monkeypatch.delenv("MACR_SEG_UNFUSED", raising=False)
    t_start = time.perf_counter()
    ranks, full = run_world(ops, world, shape, kind_name, layout, lazy)
    record_property("gpu_seconds", round(time.perf_counter() - t_start, 3))      # (the W ranks alone: the world-1 run is shared)
    base_ranks, base = world1(ops, shape, kind_name, lazy, unfused)
    want_losses, want_m1, Po, Qo, wo, wuo = reference(shape, kind_name)
    P0, Q0, w0, wu0, batches = problem(*shape)

    # ---- which path ran
    kernels = set().union(*(r["kernels"] for r in ranks))
    record_property("kernels", " ".join(sorted(kernels)))
    assert ("adam_lazy" in kernels) == (lazy > 1) and ("seg_reduce" in kernels) == unfused, kernels
    if lazy == 1:
        assert ("seg_reduce" in kernels) == unfused and ("adam_indexed" in kernels) == (not unfused), kernels
    if split:
        assert all(r["wire"][k] < 2 * 3 * B // world + 3 * B // 4 for r in ranks for k in range(steps)), [r["wire"] for r in ranks]
    else:
        assert all(r["wire"] == [None] * steps for r in ranks)            # the replicated step, not the split one

    # ---- against the CPU reference, with the project's tolerances for this path; the headroom goes on record
    worst_loss = max(float(np.abs(got / want - 1).max()) for r in ranks for got, want in zip(r["losses"], want_losses))
    tol = 2e-3 * LR * steps
    worst_tab = max(float(np.abs(full["P"] - Po).max()), float(np.abs(full["Q"] - Qo).max()),
                    max(float(np.abs(r["w"][-1] - wo).max()) for r in ranks), max(float(np.abs(r["wu"][-1] - wuo).max()) for r in ranks))
    record_property("worst_loss_rel", worst_loss)
    record_property("worst_table_abs", worst_tab)
    record_property("table_tol", tol)
    print("%s W=%d: worst loss rel %.3g (1e-5), worst table abs %.3g (%.3g)" % (shape, world, worst_loss, worst_tab, tol))
    for r in ranks:                                                         # losses on EVERY rank
        for got, want in zip(r["losses"], want_losses):
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    for name, got, want in (("mP", full["m1P"], want_m1[0]), ("mQ", full["m1Q"], want_m1[1])):
        np.testing.assert_allclose(got / 0.1, want / 0.1, rtol=2e-4, atol=2e-6 * np.abs(want / 0.1).max(), err_msg=name)
    for name, got, want in (("P", full["P"], Po), ("Q", full["Q"], Qo)):
        np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=name)
    for r in ranks:
        np.testing.assert_allclose(r["w"][-1], wo, rtol=0, atol=tol)
        np.testing.assert_allclose(r["wu"][-1], wuo, rtol=0, atol=tol)

    # ---- exact properties: the ranks of one run agree bit for bit after every step
    for r in ranks[1:]:
        for k in range(steps):
            assert np.array_equal(r["losses"][k].view(np.uint32), ranks[0]["losses"][k].view(np.uint32)), "losses differ across ranks"
            assert np.array_equal(r["w"][k].view(np.uint32), ranks[0]["w"][k].view(np.uint32)), "w differs across ranks"
            assert np.array_equal(r["wu"][k].view(np.uint32), ranks[0]["wu"][k].view(np.uint32)), "w_user differs across ranks"
    if pair:                                                                # no branch vector is trained
        assert all(np.array_equal(r["w"][k].view(np.uint32), w0.view(np.uint32)) and
                   np.array_equal(r["wu"][k].view(np.uint32), wu0.view(np.uint32)) for r in ranks for k in range(steps))
    elif kind_name == ITEM:
        assert all(np.array_equal(r["wu"][k].view(np.uint32), wu0.view(np.uint32)) for r in ranks for k in range(steps))

    # ---- W-invariance against the same entry points at world = 1 (see the module docstring)
    limit = 0 if unfused else ATOMIC_FREE_REFS
    refs = max_refs(shape)
    branch_free = pair or -(-B // (1024 // d)) <= 16                             # at most two backward blocks per partial row of dw
    atomic_free = branch_free and all(cu.max() <= limit and ci.max() <= limit for cu, ci in refs)
    calm_u, calm_i = refs[0][0] <= max(limit, 2), refs[0][1] <= max(limit, 2)     # (two addends commute whatever the chunking)
    b0 = base_ranks[0]
    first_rows_equal = (np.array_equal(full["m1P"][calm_u], base["m1P"][calm_u]) and np.array_equal(full["m1Q"][calm_i], base["m1Q"][calm_i]))
    record_property("first_step_rows_bit_equal_world1", bool(first_rows_equal))
    record_property("atomic_free_batches", bool(atomic_free))
    record_property("first_step_losses_bit_equal_world1", bool(np.array_equal(ranks[0]["losses"][0], b0["losses"][0])))
    # split or not: a position's gradient rows come from its forward scalars and the row / column sums, which the slices and the
    # row blocks of the ranks reproduce exactly (x + 0), by the same arithmetic per position; the owner sums them in list order
    assert first_rows_equal, "first-step gradient rows depend on W"
    if not split:                                       # (split: the loss partials are cut per slice -- on record above, tolerance)
        assert np.array_equal(ranks[0]["losses"][0], b0["losses"][0]), "first-step losses depend on W"
        first_w_equal = np.array_equal(ranks[0]["w"][0], b0["w"][0]) and np.array_equal(ranks[0]["wu"][0], b0["wu"][0])
        record_property("first_step_branch_vectors_bit_equal_world1", bool(first_w_equal))
        assert first_w_equal or not branch_free, "first-step branch vectors depend on W"
        if atomic_free:
            for k in range(steps):
                assert np.array_equal(ranks[0]["losses"][k], b0["losses"][k]), "step %d: losses depend on W" % k
                assert np.array_equal(ranks[0]["w"][k], b0["w"][k]) and np.array_equal(ranks[0]["wu"][k], b0["wu"][k])
            for name in ("P", "Q", "mP", "vP", "mQ", "vQ"):
                assert np.array_equal(full[name], base[name]), "%s depends on W" % name
