"""Self-check of the in-process world (tests/shard_loopback.py) on the CPU: W threads, the ORACLE as the device half
(OracleBackend / SplitOracleBackend of tests/test_sharded_train_cpu.py), the production RowShardedMF.step / step_split.
What the gloo rigs of that file assert at 2 and 3 ranks must hold at 2, 3, 8 and 16: losses within 1e-6 of the single-process
oracle step, the reassembled tables and every rank's branch vectors equal to the oracle's bit for bit -- so that the harness is
known exact before tests/test_gpu_shard_worlds.py trusts it on the GPU.  The "few" problem has fewer user rows than ranks:
some ranks own no row of P."""
import functools
import threading

import numpy as np
import pytest
import torch

import oracle
import shard_loopback
from macr_amd import sharded_train
from test_sharded_train_cpu import HYP, OracleBackend, SplitOracleBackend

KINDS = {"rubibceboth": oracle.LOSS_RUBIBCEBOTH, "rubibce": oracle.LOSS_RUBIBCE, "normalbce": oracle.LOSS_NORMALBCE}
SHAPES = {"wide": (301, 77), "few": (5, 77)}          # (n_users, n_items)
D, B, STEPS = 16, 96, 3


@functools.lru_cache(maxsize=None)
def problem(shape):
    n_users, n_items = SHAPES[shape]
    rs = np.random.RandomState(12 + n_users)
    P = (rs.standard_normal((n_users, D)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((n_items, D)) * 0.3).astype(np.float32)
    w, wu = (rs.standard_normal(D) * 0.3).astype(np.float32), (rs.standard_normal(D) * 0.3).astype(np.float32)
    batches = []
    for _ in range(STEPS):
        u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
        i = (rs.zipf(1.3, B) % n_items).astype(np.int32)
        j = rs.randint(0, n_items, B).astype(np.int32)
        batches.append((u, i, j))
    return P, Q, w, wu, batches


@functools.lru_cache(maxsize=None)
def expected(shape, kind_name):
    """the single-process oracle run: (losses per step, P, Q, w, wu) -- computed once per problem and kind, never written to"""
    P, Q, w, wu, batches = problem(shape)
    Po, Qo, wo, wuo = P.copy(), Q.copy(), w.copy(), wu.copy()
    st = oracle.AdamState([P.shape, Q.shape, w.shape, wu.shape])
    losses = [oracle.mf_train_step(KINDS[kind_name], u, i, j, Po, Qo, wo, wuo, st, HYP["lr"], HYP["decay"], HYP["alpha"],
                                   HYP["beta"], HYP["bs"]).copy() for u, i, j in batches]
    for a in (Po, Qo, wo, wuo):
        a.setflags(write=False)
    return losses, Po, Qo, wo, wuo


def run_world(world, shape, kind_name, layout, split):
    P, Q, w, wu, batches = problem(shape)
    backend = SplitOracleBackend if split else OracleBackend

    def rank_main(rank, comm):
        model = shard_loopback.LoopbackMF(comm, rank, torch.from_numpy(P), torch.from_numpy(Q), torch.from_numpy(w),
                                          torch.from_numpy(wu), backend(KINDS[kind_name], D, **HYP), layout=layout)
        losses, wire = [], []
        for u, i, j in batches:
            losses.append(model.step(torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(j)).numpy().copy())
            wire.append(model.wire_rows)
        return dict(losses=losses, wire=wire, P=model.P, Q=model.Q, w=model.w.numpy(), wu=model.wu.numpy(),
                    own_u=model.own_u, own_i=model.own_i)

    return shard_loopback.run_ranks(world, rank_main, timeout=60.0)


CASES = [(W, "wide", k, lay, s) for W in (2, 3, 8, 16) for lay in ("interleaved", "range")
         for k, s in (("normalbce", False), ("rubibce", False), ("rubibceboth", False), ("rubibce", True), ("rubibceboth", True))]
CASES += [(W, "few", k, lay, s) for W in (8, 16) for lay in ("interleaved", "range")
          for k, s in (("normalbce", False), ("rubibceboth", False), ("rubibceboth", True))]


@pytest.mark.parametrize("world,shape,kind_name,layout,split", CASES)
def test_loopback_world_reproduces_the_oracle_step(world, shape, kind_name, layout, split):
    want_losses, Po, Qo, wo, wuo = expected(shape, kind_name)
    ranks = run_world(world, shape, kind_name, layout, split)
    n_users, n_items = SHAPES[shape]
    if shape == "few":
        assert sum(r["own_u"].n == 0 for r in ranks) >= world - n_users          # ranks without a user row
    for r in ranks:
        for got, want in zip(r["losses"], want_losses):
            np.testing.assert_allclose(got, want, rtol=1e-6)
        assert np.array_equal(r["w"], wo) and np.array_equal(r["wu"], wuo)
        if split:
            assert max(r["wire"]) < 2 * 3 * B // world + 3 * B // 4
        else:
            assert r["wire"] == [None] * STEPS                                    # the replicated step ran, not the split one
    Pf = shard_loopback.reassemble([r["P"] for r in ranks], [r["own_u"] for r in ranks], n_users)
    Qf = shard_loopback.reassemble([r["Q"] for r in ranks], [r["own_i"] for r in ranks], n_items)
    assert np.array_equal(Pf.numpy(), Po) and np.array_equal(Qf.numpy(), Qo)


def test_loopback_collectives():
    """the three exchanges themselves, on tensors whose sum depends on the order: rank order, identical on every rank"""
    W = 5
    vals = [torch.tensor([1e8, 1.0, -1e8, 3.0 * r], dtype=torch.float32) * (r + 1) for r in range(W)]
    want = vals[0].clone()
    for r in range(1, W):
        want += vals[r]
    counts = [[(q + 2 * p) % 3 for p in range(W)] for q in range(W)]            # counts[q][p]: rows q sends to p

    def rank_main(rank, comm):
        t = vals[rank].clone()
        comm.all_reduce(rank, t)
        b = torch.full((3,), float(rank))
        comm.broadcast(rank, b, 2)
        send = torch.tensor([[100.0 * rank + p] for p in range(W) for _ in range(counts[rank][p])]).reshape(-1, 1)
        recv_counts = [counts[q][rank] for q in range(W)]
        recv = torch.full((sum(recv_counts), 1), -1.0)
        comm.all_to_all(rank, recv, send, recv_counts, counts[rank])
        return t, b, recv

    for rank, (t, b, recv) in enumerate(shard_loopback.run_ranks(W, rank_main, timeout=30.0)):
        assert torch.equal(t, want) and torch.equal(b, torch.full((3,), 2.0))
        assert recv.reshape(-1).tolist() == [100.0 * q + rank for q in range(W) for _ in range(counts[q][rank])]


def test_loopback_first_error_stops_every_rank():
    """a rank that raises aborts the barrier: the others leave their collective at once, the first exception comes back"""
    passed = []

    def rank_main(rank, comm):
        t = torch.ones(2)
        comm.all_reduce(rank, t)
        if rank == 1:
            raise ValueError("rank 1 gives up")
        comm.all_reduce(rank, t)                                                 # never completes: rank 1 is gone
        passed.append(rank)

    with pytest.raises(RuntimeError, match="rank 1 of 4: ValueError: rank 1 gives up") as info:
        shard_loopback.run_ranks(4, rank_main, timeout=30.0)
    assert isinstance(info.value.__cause__, ValueError) and not passed
    assert threading.active_count() == 1 or all(not th.name.startswith("rank") for th in threading.enumerate())
