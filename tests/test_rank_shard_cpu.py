"""The item-sharded position count without a GPU: the NumPy restatement of the three calls (tests/rank_shard_ref.py) against
the unsharded restatement (tests/rank_ref.py) for every shard shape; sharding.sum_over_ranks in a world of one and in a gloo
world of two; the environment switch; the entry points' declarations and their refusals, which come before any device work
(the pointers below are never dereferenced, as in tests/test_rank_positions_cpu.py)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_ref
import rank_shard_ref
from helpers import REPO
from test_gpu_rank_positions import lists          # the pair and mask lists of the unsharded GPU tests (NumPy only)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("layout", ["interleaved", "range"])
@pytest.mark.parametrize("n_items", [31, 129, 333])
def test_summed_shard_counts_are_the_unsharded_positions(n_items, layout):
    rs = np.random.RandomState(7 * n_items + len(layout))
    U = 23
    scores = rs.standard_normal((U, n_items)).astype(np.float32)
    scores[:, 5] = scores[:, 17]                               # ties across shards
    scores[3] = 0.0                                            # a row of nothing but ties
    scores[4, ::2] = -0.0
    scores[4, 1::2] = 0.0
    scores[:, 11] = np.nan
    pairs, mask = lists(rs, U, n_items)
    pairs[5] = sorted(set(pairs[5]) | {5, 11, 17})
    want = rank_ref.positions(scores, mask, pairs)
    assert -1 in want and want.max() > n_items // 2
    for world in (1, 2, 3, 5, 16):
        parts = rank_shard_ref.shards(n_items, world, layout)
        assert sorted(g for s in parts for g in rank_shard_ref.owned(s).tolist()) == list(range(n_items))      # a partition
        got = rank_shard_ref.positions(scores, world, layout, mask, pairs)
        assert np.array_equal(got, want), (world, np.flatnonzero(got != want)[:10])


def test_shards_are_empty_when_there_are_fewer_items_than_ranks():
    for layout in ("interleaved", "range"):
        parts = rank_shard_ref.shards(5, 16, layout)
        assert sum(s[2] for s in parts) == 5 and [s[2] for s in parts].count(0) == 11
    rs = np.random.RandomState(2)
    scores = rs.standard_normal((4, 5)).astype(np.float32)
    pairs, mask = [[0, 4], [1], [], [2, 3, 7]], [[1], [], [0], [3]]
    for layout in ("interleaved", "range"):
        assert np.array_equal(rank_shard_ref.positions(scores, 16, layout, mask, pairs), rank_ref.positions(scores, mask, pairs))


def test_the_flag_and_the_two_empty_keys():
    scores = np.asarray([[3.0, 2.0, np.nan, 1.0]], dtype=np.float32)
    parts = rank_shard_ref.shards(4, 2, "interleaved")          # {0, 2} and {1, 3}
    pairs, mask = [[1, 2, 3, 9]], [[0, 3]]
    k0, k1 = (rank_shard_ref.shard_keys(scores, s, pairs) for s in parts)
    assert k0[0] == 0 and k0[1] == rank_shard_ref.NO_KEY and k0[2] == 0 and k0[3] == 0
    assert k1[0] != 0 and k1[1] == 0 and k1[2] != 0 and k1[3] == 0
    keys = rank_shard_ref.sum_int64([k0, k1]).view(np.uint64)
    assert keys[1] == rank_shard_ref.NO_KEY and keys[3] == 0    # NaN; nobody's item
    c0 = rank_shard_ref.shard_counts(scores, parts[0], mask, pairs, keys)
    c1 = rank_shard_ref.shard_counts(scores, parts[1], mask, pairs, keys)
    assert c0.tolist() == [0, 0, 0, 0]                          # item 0 is before both, and masked: 1 - 1
    assert c1.tolist() == [0, 0, 1 + rank_shard_ref.MASKED, 0]  # item 1 is before item 3; item 3 is masked and rank 1's
    assert rank_shard_ref.combine(keys, c0 + c1).tolist() == [0, -1, -1, -1]


# ----------------------------------------------------------------------------- sharding.sum_over_ranks
def test_sum_over_ranks_is_the_identity_in_a_world_of_one(monkeypatch):
    from macr_amd import sharding
    monkeypatch.delenv("MACR_FORCE_COLLECTIVES", raising=False)
    t = torch.tensor([0, -1, 1 << 62, -(1 << 63)], dtype=torch.int64)
    assert sharding.sum_over_ranks(t) is t
    with pytest.raises(TypeError):
        sharding.sum_over_ranks(t.to(torch.int32))


def _sum_worker(rank, world, port, q):
    from macr_amd import sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # keys: x + 0 with the top bit set and all ones (-1 as int64); counts: plain integers and the flag from one rank
        mine = [[-1, 0, -(1 << 63) + 5, 7, 1 << 40], [0, (1 << 63) - 1, 0, 1 << 30, 3]][rank]
        t = torch.tensor(mine, dtype=torch.int64)
        out = sharding.sum_over_ranks(t)
        q.put((rank, out.tolist(), t.tolist() == mine))
    finally:
        dist.destroy_process_group()


def test_sum_over_ranks_gloo_world2_keeps_every_bit():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sum_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=60) for _ in procs)
    for p in procs:
        p.join(60)
    want = [-1, (1 << 63) - 1, -(1 << 63) + 5, 7 + (1 << 30), (1 << 40) + 3]
    assert [r[1] for r in res] == [want, want]
    assert [r[2] for r in res] == [True, True]                  # the operand is left as it was


# ----------------------------------------------------------------------------- the switch
def test_shard_rank_report_switch_is_the_environment(monkeypatch):
    from macr_amd import rank_report
    monkeypatch.delenv("MACR_RANK_REPORT", raising=False)
    monkeypatch.delenv("MACR_SHARD_RANK_REPORT", raising=False)
    assert not rank_report.shard_enabled() and not rank_report.wanted()
    monkeypatch.setenv("MACR_SHARD_RANK_REPORT", "0")
    assert not rank_report.shard_enabled()
    monkeypatch.setenv("MACR_SHARD_RANK_REPORT", "1")
    assert rank_report.shard_enabled() and rank_report.wanted() and not rank_report.enabled()
    monkeypatch.setenv("MACR_RANK_REPORT", "1")
    monkeypatch.delenv("MACR_SHARD_RANK_REPORT")
    assert rank_report.enabled() and rank_report.wanted() and not rank_report.shard_enabled()
    for path in ("macr_mf/parse.py", "macr_lightgcn/utility/parser.py"):                 # no parser flag
        assert "rank_report" not in open(os.path.join(REPO, path)).read().lower()


# ----------------------------------------------------------------------------- the C ABI
U, N, D, NP = 300, 2500, 64, 1234


@pytest.fixture(scope="module")
def lib():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    """a 256-byte aligned host address standing in for every buffer"""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, base


def test_entry_points_and_the_flag_constant(lib):
    import re
    L = lib.lib()
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    assert int(re.search(r"#define MACR_RANK_SHARD_MASKED \(1LL << (\d+)\)", src).group(1)) == 40
    assert lib.RANK_SHARD_MASKED == 1 << 40 == rank_shard_ref.MASKED
    for name, n_args in (("macr_rank_shard_workspace_bytes", 4), ("macr_rank_shard_keys", 18), ("macr_rank_shard_counts", 22),
                         ("macr_rank_shard_combine", 5)):
        assert hasattr(L, name) and len(lib.SIGNATURES[name][1]) == n_args, name
    # the existing calls keep their signatures
    assert len(lib.SIGNATURES["macr_score_pairs"][1]) == 16 and len(lib.SIGNATURES["macr_rank_positions"][1]) == 20


def keys_call(lib, mem, **over):
    p = ctypes.c_void_p(mem[1])
    a = dict(kind=lib.SCORE_RUBI_BOTH, U=U, N=N, d=D, users=p, user_ids=p, items=p, sig_u=p, sig_i=p, c=0.5, c_dev=None, lo=3,
             stride=5, pair_ptr=p, pair_item=p, n_pairs=NP, out=p)
    a.update(over)
    return lib.lib().macr_rank_shard_keys(a["kind"], a["U"], a["N"], a["d"], a["users"], a["user_ids"], a["items"], a["sig_u"],
                                          a["sig_i"], a["c"], a["c_dev"], a["lo"], a["stride"], a["pair_ptr"], a["pair_item"],
                                          a["n_pairs"], a["out"], None)


def counts_call(lib, mem, **over):
    p = ctypes.c_void_p(mem[1])
    L = lib.lib()
    a = dict(kind=lib.SCORE_RUBI_BOTH, U=U, N=N, d=D, users=p, user_ids=p, items=p, sig_u=p, sig_i=p, c=0.5, c_dev=None, lo=3,
             stride=5, mask_ptr=p, mask_idx=p, pair_ptr=p, keys=p, n_pairs=NP, out=p, ws=p, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.macr_rank_shard_workspace_bytes(U, NP, N, D)
    return L.macr_rank_shard_counts(a["kind"], a["U"], a["N"], a["d"], a["users"], a["user_ids"], a["items"], a["sig_u"],
                                    a["sig_i"], a["c"], a["c_dev"], a["lo"], a["stride"], a["mask_ptr"], a["mask_idx"],
                                    a["pair_ptr"], a["keys"], a["n_pairs"], a["out"], a["ws"], a["ws_bytes"], None)


def test_shard_calls_refuse_with_their_documented_codes(lib, mem):
    L = lib.lib()
    need = L.macr_rank_shard_workspace_bytes(U, NP, N, D)
    common = [
        ("no kind at all", dict(kind=5), lib.E_INVALID, b"score_kind=5"),
        ("d = 48", dict(d=48), lib.E_UNSUPPORTED, b"d=48"),
        ("no queries", dict(U=0), lib.E_INVALID, b"U=0"),
        ("an empty shard", dict(N=0), lib.E_INVALID, b"n_local=0"),
        ("a negative pair count", dict(n_pairs=-1), lib.E_INVALID, b"n_pairs=-1"),
        ("more pairs than an int32 CSR holds", dict(n_pairs=1 << 31), lib.E_INVALID, b"n_pairs=2147483648"),
        ("no stride", dict(stride=0), lib.E_INVALID, b"item_stride=0"),
        ("a negative stride", dict(stride=-2), lib.E_INVALID, b"item_stride=-2"),
        ("a negative first item", dict(lo=-1), lib.E_INVALID, b"item_lo=-1"),
        ("no user table", dict(users=None), lib.E_INVALID, b"null pointer"),
        ("no item table", dict(items=None), lib.E_INVALID, b"null pointer"),
        ("no pair CSR", dict(pair_ptr=None), lib.E_INVALID, b"null pointer"),
        ("RUBI_BOTH without sig_u", dict(sig_u=None), lib.E_INVALID, b"sig_u"),
        ("RUBI without sig_i", dict(kind=lib.SCORE_RUBI, sig_i=None), lib.E_INVALID, b"sig_i"),
    ]
    for name, over, code, text in common + [("no pair items", dict(pair_item=None), lib.E_INVALID, b"null pointer"),
                                            ("no output", dict(out=None), lib.E_INVALID, b"out_keys")]:
        rc = keys_call(lib, mem, **over)
        msg = L.macr_last_error()
        assert rc == code and b"rank_shard_keys" in msg and text in msg, (name, rc, msg)
    for name, over, code, text in common + [
            ("no keys", dict(keys=None), lib.E_INVALID, b"null pointer"),
            ("half a mask", dict(mask_idx=None), lib.E_INVALID, b"mask_ptr and mask_idx"),
            ("no output", dict(out=None), lib.E_INVALID, b"out_cnt"),
            ("no workspace", dict(ws=None), lib.E_INVALID, b"workspace"),
            ("an unaligned workspace", dict(ws=ctypes.c_void_p(mem[1] + 8)), lib.E_INVALID, b"workspace"),
            ("a workspace one byte short", dict(ws_bytes=need - 1), lib.E_WORKSPACE, b"workspace")]:
        rc = counts_call(lib, mem, **over)
        msg = L.macr_last_error()
        assert rc == code and b"rank_shard_counts" in msg and text in msg, (name, rc, msg)
    # nothing to rank: no device work, no outputs needed
    assert keys_call(lib, mem, n_pairs=0, out=None, pair_item=None) == lib.OK
    assert counts_call(lib, mem, n_pairs=0, out=None, keys=None) == lib.OK
    p = ctypes.c_void_p(mem[1])
    assert L.macr_rank_shard_combine(0, None, None, None, None) == lib.OK
    assert L.macr_rank_shard_combine(-1, p, p, p, None) == lib.E_INVALID and b"n_pairs=-1" in L.macr_last_error()
    assert L.macr_rank_shard_combine(5, p, None, p, None) == lib.E_INVALID and b"rank_shard_combine" in L.macr_last_error()


def test_shard_workspace_size(lib):
    ws, whole = lib.lib().macr_rank_shard_workspace_bytes, lib.lib().macr_rank_positions_workspace_bytes
    for bad in [(U, NP, N, 48), (0, NP, N, D), (U, -1, N, D), (U, NP, 0, D), (U, 1 << 31, N, D)]:
        assert ws(*bad) == 0, bad
    for p in (0, 1, 16, 17, 1000, 123456):
        assert ws(U, p, N, D) % 16 == 0 and 0 < ws(U, p, N, D) <= whole(U, p, N, D)
        assert whole(U, p, N, D) - ws(U, p, N, D) == (p * 8 + 15) // 16 * 16         # the keys are the caller's
        assert ws(U, p, N, D) == ws(U, p, N + 7, D)
