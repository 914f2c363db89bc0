"""An in-process world for macr_amd.sharded_train.RowShardedMF: W ranks as W Python threads of ONE process.

RowShardedMF does all of its communication through _all_reduce / _broadcast / _all_to_all.  LoopbackMF overrides those three
with exchanges through a shared Loopback object built on threading.Barrier, so that the production step() / step_split() run
unchanged for any W <= 16 without a process launch per rank -- on the CPU with the oracle as the device half
(tests/test_shard_loopback_cpu.py proves the harness exact) and on one GPU with the HIP backend (tests/test_gpu_shard_worlds.py).

On the GPU every thread uses the default stream of the one context: work is ordered by the order the host submits it in, and
the barriers order the host, so a collective reads its peers' buffers after the kernels that fill them were enqueued.

    all_reduce   the W tensors summed in rank order 0 .. W-1, once; every rank copies the one result (identical, deterministic)
    broadcast    a copy of src's tensor
    all_to_all   rank q's rows [sum(send_counts_q[:p]), +send_counts_q[p]) land behind what ranks < q sent to p

An exception in any rank aborts the barrier: the others stop at their next collective (BrokenBarrierError), nothing is retried,
and run_ranks re-raises the FIRST exception after joining every thread."""
import threading

import torch

from macr_amd import sharded_train


class Loopback(object):
    def __init__(self, world, timeout=120.0):
        if not 1 <= world <= 16:
            raise ValueError("loopback world of %d ranks (1 .. 16)" % world)
        self.world = world
        self.barrier = threading.Barrier(world, timeout=timeout)
        self.slots = [None] * world
        self.result = None

    def all_reduce(self, rank, t):
        self.slots[rank] = t
        if self.barrier.wait() == 0:                      # exactly one thread sums, in rank order
            acc = self.slots[0].clone()
            for r in range(1, self.world):
                acc += self.slots[r]
            self.result = acc
        self.barrier.wait()
        t.copy_(self.result)
        self.barrier.wait()                               # nobody posts the next collective before everybody has read this one

    def broadcast(self, rank, t, src):
        if rank == src:
            self.slots[src] = t
        self.barrier.wait()
        if rank != src:
            t.copy_(self.slots[src])
        self.barrier.wait()

    def all_to_all(self, rank, recv, send, recv_counts, send_counts):
        assert send.shape[0] == sum(send_counts) and recv.shape[0] == sum(recv_counts)
        self.slots[rank] = (send, list(send_counts))
        self.barrier.wait()
        at = 0
        for q in range(self.world):
            rows, counts = self.slots[q]
            n, off = counts[rank], sum(counts[:rank])
            assert n == recv_counts[q], "rank %d expects %d rows of rank %d, which sends %d" % (rank, recv_counts[q], q, n)
            recv[at:at + n] = rows[off:off + n]
            at += n
        self.barrier.wait()


class LoopbackMF(sharded_train.RowShardedMF):
    """RowShardedMF whose three collectives go through a Loopback (everything else is the production class)"""

    def __init__(self, comm, rank, *args, **kwargs):
        self.comm = comm
        super(LoopbackMF, self).__init__(*args, rank=rank, world=comm.world, **kwargs)

    def _all_reduce(self, t, name="all_reduce"):
        self.comm.all_reduce(self.rank, t)

    def _broadcast(self, t, src=0, name="broadcast"):
        self.comm.broadcast(self.rank, t, src)

    def _all_to_all(self, recv, send, recv_counts, send_counts, name):
        self.comm.all_to_all(self.rank, recv, send, recv_counts, send_counts)


def run_ranks(world, fn, timeout=120.0):
    """fn(rank, comm) on `world` threads sharing one Loopback -> [fn's result of rank 0, .., of rank world-1].
    The first exception of any rank is re-raised here, after every thread has ended."""
    comm = Loopback(world, timeout)
    results, errors, lock = [None] * world, [], threading.Lock()

    def target(rank):
        try:
            results[rank] = fn(rank, comm)
        except BaseException as e:                        # noqa: B902 -- whatever it is, the other ranks must stop
            with lock:
                errors.append((rank, e))
            comm.barrier.abort()

    if world == 1:
        return [fn(0, comm)]                              # the caller's own thread: its exceptions (an interrupt too) pass unchanged
    threads = [threading.Thread(target=target, args=(r,), name="rank%d" % r) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        first = [e for e in errors if not isinstance(e[1], threading.BrokenBarrierError)] or errors
        rank, exc = first[0]
        raise RuntimeError("rank %d of %d: %s: %s" % (rank, world, type(exc).__name__, exc)) from exc
    return results


def reassemble(shards, owners, n_rows):
    """full (n_rows, d) table from every rank's rows (torch tensors) and Owned layouts; asserts that every row is owned exactly
    once"""
    d = next(s.shape[1] for s in shards)
    full = torch.zeros((n_rows, d), dtype=shards[0].dtype)
    seen = torch.zeros(n_rows, dtype=torch.int64)
    for rows, own in zip(shards, owners):
        assert rows.shape[0] == own.n
        ids = own.global_ids()
        full[ids] = rows.cpu()
        seen[ids] += 1
    assert bool((seen == 1).all()), "rows owned %s times" % sorted(set(seen.tolist()))
    return full
