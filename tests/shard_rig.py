"""What the GPU tests of the row-sharded step's modes share (tests/test_gpu_shard_deterministic.py, tests/test_gpu_shard_invariant.py):
the problems with hand-written hot runs and their CPU restatements, collectives that add in another order, and run_world -- a
problem's steps on W ranks in the in-process worlds of tests/shard_loopback.py (W threads, one GPU context, the production
RowShardedMF.step / step_split), in any of the step's modes, with the mode's path-and-hygiene assertions inside."""
import functools
import threading

import numpy as np
import torch

import bpr_ref
import oracle
import shard_loopback

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 512
BOTH, ITEM, NORMAL, BPR = "LOSS_RUBIBCEBOTH", "LOSS_RUBIBCE", "LOSS_NORMALBCE", "LOSS_BPR"
ALL_FORMS = ((BOTH, True), (BOTH, False), (ITEM, True), (ITEM, False), (NORMAL, False), (BPR, False))      # (kind, split)
TABLES = ("P", "Q", "mP", "vP", "mQ", "vQ")
SMALL = ("mw", "vw", "mwu", "vwu")
# the modes a world can run in -> HipBackend keywords; the workspace size function and the row-sum kernels of the ordered ones
MODES = {"inv": dict(invariant=True), "det": dict(deterministic=True), "plain": {}}
WS_BYTES = {"det": "macr_shard_workspace_bytes_det", "inv": "macr_shard_workspace_bytes_inv"}
ROW_SUMS = {"det": {"seg_reduce", "seg_fold"}, "inv": {"seg_reduce_inv", "seg_fold_inv"}}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a writable copy: the problems' arrays are read-only)


def bits(a, b):
    """same shape, same bits"""
    a, b = (x.numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def set_form(monkeypatch, split):
    monkeypatch.setenv("MACR_SHARD_SPLIT", "1" if split else "0")
    for name in ("MACR_SHARD_ROUTE_TORCH", "MACR_SEG_UNFUSED", "MACR_LAZY_ADAM", "MACR_SHARD_INVARIANT", "MACR_SHARD_DETERMINISTIC"):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def problem(B, d, n_users, n_items, steps, hot):
    """tables, branch vectors and one batch per step: a fresh draw, the hot runs [(array, start, stop, row)] written over it, then
    spread over the batch's blocks by a permutation"""
    rs = np.random.RandomState(B + d + n_users)
    P = (rs.standard_normal((n_users, d)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    batches = []
    for _ in range(steps):
        b = dict(u=rs.choice(n_users, B, replace=B > n_users).astype(np.int32), i=rs.randint(0, n_items, B).astype(np.int32),
                 j=rs.randint(0, n_items, B).astype(np.int32))
        for name, lo, hi, row in hot:
            b[name][lo:hi] = row
        o = rs.permutation(B)
        batches.append(tuple(b[k][o] for k in ("u", "i", "j")))
    for a in (P, Q, w, wu) + tuple(x for b in batches for x in b):
        a.setflags(write=False)
    return P, Q, w, wu, tuple(batches)


@functools.lru_cache(maxsize=None)
def cpu_reference(B, d, n_users, n_items, steps, hot, kind_name):
    """the single-process CPU run of a problem, once: losses per step, m of P and Q after the first step, final P, Q, w, w_user"""
    P, Q, w, wu, batches = problem(B, d, n_users, n_items, steps, hot)
    if kind_name == BPR:
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


# ----------------------------------------------------------------------------- collectives that add in another order
class OrderedLoopback(shard_loopback.Loopback):
    """Loopback whose all_reduce adds the ranks' tensors in the order `order(call)` gives (broadcast and all_to_all add nothing)"""

    def __init__(self, world, timeout=120.0):
        super(OrderedLoopback, self).__init__(world, timeout)
        self.calls = 0

    def order(self, call):
        raise NotImplementedError

    def all_reduce(self, rank, t):
        self.slots[rank] = t
        if self.barrier.wait() == 0:                      # exactly one thread sums
            order = self.order(self.calls)
            self.calls += 1
            assert sorted(order) == list(range(self.world))
            acc = self.slots[order[0]].clone()
            for r in order[1:]:
                acc += self.slots[r]
            self.result = acc
        self.barrier.wait()
        t.copy_(self.result)
        self.barrier.wait()


class ReversedLoopback(OrderedLoopback):
    def order(self, call):
        return list(range(self.world - 1, -1, -1))


class RotatingLoopback(OrderedLoopback):
    def order(self, call):
        k = (call + 1) % self.world                       # (never the identity twice in a row; the first call starts at rank 1)
        return list(range(k, self.world)) + list(range(k))


_LAUNCH = threading.Lock()


def serial_backend(sharded_train):
    """HipBackend whose library calls are taken one rank at a time: the kernel timing marks of the library are one list per
    process, and W threads launch into it"""
    class SerialBackend(sharded_train.HipBackend):
        pass

    def locked(fn):
        @functools.wraps(fn)
        def call(self, *a, **kw):
            with _LAUNCH:
                return fn(self, *a, **kw)
        return call
    for name in ("gather", "lazy_rows", "lazy_flush", "forward_and_bxb", "backward", "route", "forward_slice", "bxb", "backward_slice",
                 "stage_rows", "apply", "rank_rows", "fold_ranks", "branch_fold"):
        setattr(SerialBackend, name, locked(getattr(sharded_train.HipBackend, name)))
    return SerialBackend


def run_world(ops, problem_spec, case, mode, loopback=None):
    """the steps of a problem (B, d, n_users, n_items, steps, flush after step, hot runs) as the case (kind, split, W, layout, lazy
    period) runs them, in a mode of MODES, through run_ranks' Loopback or the given one -> dict(
      ranks  per rank: `losses`, `w`, `wu` after every step; the shard's tables and slots after every flush (`flushed`: the one
             after step `flush after`, the one at the end) and at the end (by name); `m1P`, `m1Q` after the first step; the branch
             slots, `adam_pow`, the stamps `stP`, `stQ` of a lazy run, `own_u`, `own_i`; `kernels` of the last step on rank 0
      full   the tables and slots of every flush, reassembled;  m1P, m1Q  reassembled)"""
    from macr_amd import sharded_train
    B, d, n_users, n_items, steps, flush_after, hot = problem_spec
    kind_name, split, W, layout, lazy = case
    P, Q, w, wu, batches = problem(B, d, n_users, n_items, steps, hot)
    kind, device = getattr(ops, kind_name), torch.device("cuda")
    Backend = serial_backend(sharded_train)

    def tables_of(model):
        return {t: getattr(model, t).cpu() for t in TABLES}          # (the properties flush what the lazy pass left behind)

    def rank_main(rank, comm):
        hyper = ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)
        backend = Backend(kind, d, hyper, device, **MODES[mode])
        model = shard_loopback.LoopbackMF(comm, rank, dev(P), dev(Q), dev(w), dev(wu), backend, layout=layout, lazy_period=lazy)
        assert model.invariant == (mode == "inv") == backend.invariant
        assert model.deterministic == (mode == "det") == backend.deterministic
        assert model.split == split and model.lazy_period == lazy
        L = backend._lib.lib()
        if mode in WS_BYTES:
            assert getattr(L, WS_BYTES[mode])(B, d) > L.macr_shard_workspace_bytes(B, d)
        out = dict(losses=[], w=[], wu=[], own_u=model.own_u, own_i=model.own_i, flushed=[])
        for k, (u, i, j) in enumerate(batches):
            last = k == len(batches) - 1
            if last:                                    # one rank opens the timing, every rank's launches of the step go on its list
                comm.barrier.wait()
                if rank == 0:
                    ops.timing_begin()
                comm.barrier.wait()
            out["losses"].append(model.step(dev(u), dev(i), dev(j)).cpu().numpy().copy())
            if last:
                comm.barrier.wait()
                if rank == 0:
                    out["kernels"] = {n for n, _ in ops.timing_end(250)}
                comm.barrier.wait()
            out["w"].append(model.w.cpu().numpy())
            out["wu"].append(model.wu.cpu().numpy())
            if mode in WS_BYTES:                        # the gradient scratch and the row flags are left clean by every step
                assert not bool(model.gP.any()) and not bool(model.gQ.any()), "step %d: gradient scratch not zero" % k
                assert int(model.tP.sum()) == 0 and int(model.tQ.sum()) == 0, "step %d: row flags left set" % k
                assert backend.ws.numel() == getattr(L, WS_BYTES[mode])(B, d)
            if k == 0:
                out["m1P"], out["m1Q"] = model._mP.cpu(), model._mQ.cpu()
            if flush_after is not None and k + 1 == flush_after:
                model.flush()                           # (an evaluation, a checkpoint: every row brought to the current step)
                out["flushed"].append(tables_of(model))
        out["flushed"].append(tables_of(model))
        out.update(out["flushed"][-1])
        for name in SMALL:
            out[name] = getattr(model, name).cpu()
        out["adam_pow"] = backend.adam_pow.cpu()
        if lazy > 1:
            out["stP"], out["stQ"] = model.stP.cpu(), model.stQ.cpu()      # the row stamps after a flush
        return out

    saved = shard_loopback.Loopback
    if loopback is not None:
        shard_loopback.Loopback = loopback              # (run_ranks builds its Loopback by this name)
    try:
        ranks = shard_loopback.run_ranks(W, rank_main, timeout=120.0)
    finally:
        shard_loopback.Loopback = saved
    own_u, own_i = [r["own_u"] for r in ranks], [r["own_i"] for r in ranks]

    def whole(shards, t):
        return shard_loopback.reassemble(shards, own_u if t.endswith("P") else own_i, n_users if t.endswith("P") else n_items)
    world = dict(ranks=ranks, m1P=whole([r["m1P"] for r in ranks], "m1P"), m1Q=whole([r["m1Q"] for r in ranks], "m1Q"),
                 full=[{t: whole([r["flushed"][f][t] for r in ranks], t) for t in TABLES} for f in range(len(ranks[0]["flushed"]))])
    if mode in ROW_SUMS:
        check_path(ranks, case, mode)
    return world


def check_path(ranks, case, mode):
    """an ordered mode ran its own kernels in the last step, and its ranks agree bit for bit after every step"""
    kind_name, split, W, layout, lazy = case
    kernels = ranks[0]["kernels"]
    assert ROW_SUMS[mode] <= kernels, kernels
    assert not kernels & ({"seg_index", "seg_sum", "adam_indexed"} | ROW_SUMS["inv" if mode == "det" else "det"]), kernels
    assert ("branch_fold" in kernels) == (kind_name not in (NORMAL, BPR)), kernels
    assert ("adam_lazy" in kernels) == (lazy > 1) and ("adam_dense" in kernels) == (lazy == 1), kernels
    assert ("fold_ranks" in kernels) == (mode == "det" and split), kernels
    for r in ranks[1:]:
        for k in range(len(r["losses"])):
            assert bits(r["losses"][k], ranks[0]["losses"][k]), "step %d: losses differ across ranks" % k
            assert bits(r["w"][k], ranks[0]["w"][k]) and bits(r["wu"][k], ranks[0]["wu"][k]), "step %d: w / w_user differ across ranks" % k
