"""Item-sharded full-catalogue positions on the GPU: macr_rank_shard_keys / _counts / _combine with W shards played one after
another on this GPU and summed by torch, against integer counting on oracle.score_matrix (tests/rank_ref.py) and against
macr_rank_positions on the whole table -- positions EQUAL; Evaluator.rank_positions_sharded on the three shard shapes the
evaluator knows against Evaluator.rank_positions; and the MACR_SHARD_RANK_REPORT=1 line of both command lines, from one
process, from two ranks and under --row_shard 1, against the MACR_RANK_REPORT=1 line of one process on the whole table."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_ref
import rank_shard_ref
import test_gpu_rank_positions as base              # its tables, lists, oracle reference and unsharded raw() call
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu

GARBAGE = base.GARBAGE
KINDS = base.KINDS
dev = base.dev


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Sharded(object):
    """the three entry points through the C ABI for one pair / mask CSR: outputs and workspace pre-filled with garbage, the
    shards of `parts` one after another, the two sums taken with torch"""

    def __init__(self, pairs, mask):
        self.U = len(pairs)
        pp, pi = base.csr_np(pairs)
        self.n_pairs = int(pp[-1])
        self.pp, self.pi = dev(pp), dev(pi)
        self.mp = self.mi = None
        if mask is not None:
            self.mp, self.mi = (dev(a) for a in base.csr_np(mask))

    def positions(self, kind, P, uid, Q, sig_u, sig_i, c, c_dev, parts, want_parts=False):
        """P, uid, sig_u, c_dev on the device; Q, sig_i NumPy: every shard takes its rows"""
        from macr_amd import _lib
        L = _lib.lib()
        n, d = self.n_pairs, Q.shape[1]
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        cv, cp = (0.0, _p(c_dev)) if c_dev is not None else (float(c), None)
        rows = []
        for shard in parts:
            ids = rank_shard_ref.owned(shard)
            rows.append((dev(Q[ids]), None if sig_i is None else dev(sig_i[ids])) if shard[2] else None)
        keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        for shard, r in zip(parts, rows):
            if r is None:
                continue                              # an empty shard contributes zeros without a call
            out = torch.full((n,), GARBAGE, dtype=torch.int64, device="cuda")
            _lib.check(L.macr_rank_shard_keys(kind, self.U, shard[2], d, _p(P), _p(uid), _p(r[0]), _p(sig_u), _p(r[1]), cv, cp,
                                              shard[0], shard[1], _p(self.pp), _p(self.pi), n, _p(out), st))
            keys += out
        counts, per_shard = torch.zeros(n, dtype=torch.int64, device="cuda"), []
        for shard, r in zip(parts, rows):
            if r is None:
                continue
            need = L.macr_rank_shard_workspace_bytes(self.U, n, shard[2], d)
            assert need > 0
            ws = torch.full((need,), 0x5a, dtype=torch.uint8, device="cuda")
            out = torch.full((n,), GARBAGE, dtype=torch.int64, device="cuda")
            _lib.check(L.macr_rank_shard_counts(kind, self.U, shard[2], d, _p(P), _p(uid), _p(r[0]), _p(sig_u), _p(r[1]), cv, cp,
                                                shard[0], shard[1], _p(self.mp), _p(self.mi), _p(self.pp), _p(keys), n, _p(out),
                                                _p(ws), need, st))
            counts += out
            per_shard.append(out)
        pos = torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda")
        _lib.check(L.macr_rank_shard_combine(n, _p(keys), _p(counts), _p(pos), st))
        pos = pos.cpu().numpy()
        return (pos, keys.cpu().numpy(), [o.cpu().numpy() for o in per_shard]) if want_parts else pos


SHARDINGS = [(w, layout) for w in (1, 2, 3, 5) for layout in ("interleaved", "range")]


def check(ops, kind_name, P, uid, Q, w, wu, c, use_c_dev, mask, pairs, shardings, rig=None, whole=True):
    """every sharding of `shardings` gives the oracle's positions, and macr_rank_positions' on the whole table"""
    scores, sig_u, sig_i = base.reference(kind_name, P, uid, Q, w, wu, c)
    want = rank_ref.positions(scores, mask or [[]] * len(pairs), pairs)
    kind = getattr(ops, kind_name)
    opt = lambda a: None if a is None else dev(a)
    c_dev = dev(np.asarray([c], dtype=np.float32)) if use_c_dev else None
    Pd, ud, su = dev(P), opt(uid), opt(sig_u)
    if whole:
        unsharded, _ = base.raw(ops, kind, Pd, ud, dev(Q), su, opt(sig_i), c, c_dev, mask, pairs)
        assert np.array_equal(unsharded, want), kind_name
    rig = rig or Sharded(pairs, mask)
    for world, layout in shardings:
        parts = rank_shard_ref.shards(Q.shape[0], world, layout)
        pos = rig.positions(kind, Pd, ud, Q, su, sig_i, c, c_dev, parts)
        bad = np.flatnonzero(pos != want)
        assert len(bad) == 0, (kind_name, world, layout, bad[:10], pos[bad][:10], want[bad][:10])
    return want


# ----------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("n_items", [31, 129, 333])        # shards below one tile; a shard that ends a row past a tile edge
def test_sharded_positions_equal_the_oracle_and_the_unsharded_call(ops, n_items, d):
    rs = np.random.RandomState(1000 * n_items + d)
    U, n_tab = 37, 100
    P, Q, w, wu = base.tables(rs, n_tab, n_items, d)
    pairs, mask = base.lists(rs, U, n_items)
    perm = rs.permutation(n_tab)[:U].astype(np.int32)
    rig, seen = Sharded(pairs, mask), set()
    for kind_name in KINDS:
        # a permutation into the 100-row table with c by value; the table's first rows as they are with c on the device
        want = check(ops, kind_name, P, perm, Q, w, wu, 0.7, False, mask, pairs, SHARDINGS, rig)
        check(ops, kind_name, P[:U].copy(), None, Q, w, wu, -1.3, True, mask, pairs, SHARDINGS, rig)
        seen |= set(want.tolist())
    assert -1 in seen and max(seen) > min(n_items // 2, 100)


def test_ties_are_broken_by_global_id(ops):
    rs = np.random.RandomState(5)
    U, n_items, d = 37, 129, 32
    P, Q, w, wu = base.tables(rs, U, n_items, d)
    pairs, mask = base.lists(rs, U, n_items)
    two = [(3, "interleaved"), (2, "range")]
    # an all-zero item table: every score is 0.0, a pair's position is the number of unmasked smaller GLOBAL ids
    want = check(ops, "SCORE_NORMAL", P, None, np.zeros_like(Q), w, wu, 0.0, False, mask, pairs, two)
    k = 0
    for q in range(U):
        for g in pairs[q]:
            assert want[k] == (g - sum(1 for m in mask[q] if m < g) if 0 <= g < n_items and g not in mask[q] else -1), (q, g)
            k += 1
    # seven distinct rows repeated over the catalogue, also through the branch factors
    dup = Q[np.arange(n_items) % 7].copy()
    for kind_name in ("SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_DIRECT_MINUS"):
        check(ops, kind_name, P, None, dup, w, wu, 0.4, True, mask, pairs, two)
    # -0.0 and +0.0 tie; a NaN row ranks before nothing and its pairs have no position, whatever the other shards counted
    odd = Q.copy()
    odd[5] = 0.0
    odd[9] = -0.0
    odd[11] = np.nan
    pairs2 = [sorted(set(row) | {5, 9, 11}) for row in pairs]
    want = check(ops, "SCORE_NORMAL", P, None, odd, w, wu, 0.0, False, mask, pairs2, two)
    flat = np.asarray([g for row in pairs2 for g in row])
    assert np.all(want[flat == 11] == -1)
    parts = rank_shard_ref.shards(n_items, 3, "interleaved")
    pos, keys, per_shard = Sharded(pairs2, mask).positions(ops.SCORE_NORMAL, dev(P), None, odd, None, None, 0.0, None, parts, True)
    assert np.all(keys[flat == 11] == -1) and np.all(sum(per_shard)[flat == 11] == 0) and np.array_equal(pos, want)


def test_masks(ops):
    rs = np.random.RandomState(6)
    U, n_items, d = 37, 129, 64
    P, Q, w, wu = base.tables(rs, U, n_items, d)
    pairs, mask = base.lists(rs, U, n_items)               # masks of 0, 3 and N - 1 items; every seventh masks a pair item of its own
    assert any(len(m) >= n_items - 1 for m in mask) and any(set(mask[q]) & set(pairs[q]) for q in range(U))
    for q in range(0, U, 4):                                # ids outside [0, N), and an entry twice
        mask[q] = sorted(mask[q] + [-3, n_items, n_items + 5] + mask[q][:1])
    two = [(3, "interleaved"), (2, "range"), (5, "interleaved")]
    for kind_name in ("SCORE_NORMAL", "SCORE_RUBI_BOTH"):
        check(ops, kind_name, P, None, Q, w, wu, 0.7, False, mask, pairs, two)
    # the owner of a masked pair item flags it, the other shards count as for any other pair
    parts = rank_shard_ref.shards(n_items, 3, "interleaved")
    scores, _, _ = base.reference("SCORE_NORMAL", P, None, Q, w, wu, 0.0)
    pos, keys, per_shard = Sharded(pairs, mask).positions(ops.SCORE_NORMAL, dev(P), None, Q, None, None, 0.0, None, parts, True)
    assert np.array_equal(keys.view(np.uint64), rank_shard_ref.sum_int64(
        [rank_shard_ref.shard_keys(scores, s, pairs) for s in parts]).view(np.uint64))
    flagged = 0
    for s, got in zip(parts, per_shard):
        assert np.array_equal(got, rank_shard_ref.shard_counts(scores, s, mask, pairs, keys.view(np.uint64))), s
        flagged += int(((got & rank_shard_ref.MASKED) != 0).sum())
    assert flagged == sum(len(set(mask[q]) & set(pairs[q]) & set(range(n_items))) for q in range(U)) > 0
    # without a mask: only the ids outside the catalogue have no position
    want = check(ops, "SCORE_RUBI_BOTH", P, None, Q, w, wu, 0.7, False, None, pairs, two)
    flat = np.asarray([g for row in pairs for g in row])
    assert np.array_equal(want == -1, (flat < 0) | (flat >= n_items))


def test_many_tiles_and_positions_above_2_16(ops):
    rs = np.random.RandomState(9)
    U, n_items, d = 8, 70001, 32
    P, Q, w, wu = base.tables(rs, U, n_items, d)
    pairs, mask = base.lists(rs, U, n_items, mask_lens=(0, 50, 3))
    pairs[7] = sorted(set(pairs[7]) | {n_items - 1, n_items - 33, 0})
    want = check(ops, "SCORE_RUBI_BOTH", P, None, Q, w, wu, 0.3, False, mask, pairs, [(3, "interleaved")])
    assert want.max() > 1 << 16


def test_refusals_on_device_buffers(ops):
    from macr_amd import _lib
    L = _lib.lib()
    U, n, d, n_pairs = 4, 50, 64, 6
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    i = lambda *vals: torch.tensor(vals, dtype=torch.int32, device="cuda")
    P, Q, Q48 = f(U, d), f(n, d), f(n, 48)
    pp, pi, mp, mi = i(0, 2, 3, 5, 6), i(1, 2, 3, 4, 5, 6), i(0, 1, 1, 1, 1), i(7)
    keys = torch.zeros(n_pairs, dtype=torch.int64, device="cuda")
    out = torch.full((n_pairs,), GARBAGE, dtype=torch.int64, device="cuda")
    need = L.macr_rank_shard_workspace_bytes(U, n_pairs, n, d)
    ws = torch.zeros(need + 32, dtype=torch.uint8, device="cuda")

    def counts(lo=0, stride=1, Q=Q, d=d, mi=mi, ws_ptr=ws.data_ptr(), ws_bytes=need):
        return L.macr_rank_shard_counts(_lib.SCORE_NORMAL, U, n, d, _p(P), None, _p(Q), None, None, 0.0, None, lo, stride, _p(mp),
                                        _p(mi), _p(pp), _p(keys), n_pairs, _p(out), ctypes.c_void_p(ws_ptr), ws_bytes, None)

    def keys_call(lo=0, stride=1, Q=Q, d=d):
        return L.macr_rank_shard_keys(_lib.SCORE_NORMAL, U, n, d, _p(P), None, _p(Q), None, None, 0.0, None, lo, stride, _p(pp),
                                      _p(pi), n_pairs, _p(out), None)
    assert counts(stride=0) == _lib.E_INVALID and keys_call(stride=0) == _lib.E_INVALID
    assert counts(lo=-1) == _lib.E_INVALID and keys_call(lo=-1) == _lib.E_INVALID
    assert counts(ws_ptr=ws.data_ptr() + 8) == _lib.E_INVALID
    assert counts(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert counts(Q=Q48, d=48) == _lib.E_UNSUPPORTED and keys_call(Q=Q48, d=48) == _lib.E_UNSUPPORTED
    assert counts(mi=None) == _lib.E_INVALID
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all())                     # refused before any device work
    assert counts() == _lib.OK and keys_call() == _lib.OK


# ----------------------------------------------------------------------------- the evaluator
class _World(object):
    """sharding.world() of a simulated rank (no process group: the phases are played one after another)"""
    def __init__(self, monkeypatch):
        self.monkeypatch = monkeypatch

    def rank(self, r, world):
        from macr_amd import sharding
        self.monkeypatch.setattr(sharding, "world", lambda: (r, world))


def _two_phases(evaluators, call_args, world=None):
    """[(evaluator, its item rows, its branch rows)] play keys -> sum -> counts -> sum -> combine"""
    from macr_amd import ops
    kind, users_tab, uid, w, wu, c = call_args

    def summed(phase):
        total = torch.zeros(evaluators[0][0].n_gt, dtype=torch.int64, device="cuda")
        for r, (ev, rows, br) in enumerate(evaluators):
            if world is not None:
                world.rank(r, len(evaluators))
            total += phase(ev, rows, br)
        return total
    keys = summed(lambda ev, rows, br: ev.rank_shard_keys(kind, users_tab, uid, rows, w, wu, c, branch=br))
    counts = summed(lambda ev, rows, br: ev.rank_shard_counts(keys, kind, users_tab, uid, rows, w, wu, c, branch=br))
    return ops.rank_shard_combine(keys, counts)


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_evaluator_sharded_positions_equal_the_whole_tables(ops, kind_name, monkeypatch):
    from macr_amd.evaluator import Evaluator
    from macr_amd.sharded_train import Owned
    rs = np.random.RandomState(21)
    U, n_users, N = 300, 320, 2000
    model = base._mf_model(rs, n_users, N)
    model.update_c(None, 0.7)
    kind = getattr(ops, kind_name)
    uid = dev(rs.permutation(n_users)[:U].astype(np.int32))
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(U)]
    gt = [sorted(rs.choice(N, rs.randint(0, 25), replace=False).tolist()) for _ in range(U)]
    for q in range(0, U, 9):
        gt[q] = sorted(set(gt[q]) | set(mask[q][:2]))       # held-out items that are train items too: no position
    Q = model.item_embedding
    args = (kind, model.user_embedding, uid, model.w, model.w_user, model.rubi_c)
    whole = Evaluator(mask, gt, N, "cuda")
    want = whole.rank_positions(kind, model.user_embedding, uid, Q, model.w, model.w_user, model.rubi_c)
    assert want.dtype == torch.int32 and want.shape == (whole.n_gt,) and int((want == -1).sum()) > 0 and int(want.max()) > N // 2
    # an unsharded evaluator in a world of one
    assert torch.equal(whole.rank_positions_sharded(kind, model.user_embedding, uid, Q, model.w, model.w_user, model.rubi_c), want)
    # strided shards (set_local_items of an interleaved Owned), three ranks
    strided = []
    for r in range(3):
        ev, own = Evaluator(mask, gt, N, "cuda"), Owned(N, r, 3)
        ev.set_local_items(own)
        strided.append((ev, own.take(Q).contiguous(), None))
    # contiguous halves the caller holds (local_items_range)
    halves = []
    for lo, hi in ((0, N // 2), (N // 2, N)):
        ev = Evaluator(mask, gt, N, "cuda")
        ev.local_items_range = (lo, hi)
        halves.append((ev, Q[lo:hi].contiguous(), None))
    for shards in (strided, halves):
        first = _two_phases(shards, args)
        assert torch.equal(first, want)
        assert torch.equal(_two_phases(shards, args), first)                # the cached workspace
    # a replicated table cut by item_shard_range: three simulated ranks
    replicated = [(Evaluator(mask, gt, N, "cuda"), Q, None) for _ in range(3)]
    assert torch.equal(_two_phases(replicated, args, _World(monkeypatch)), want)
    assert torch.equal(_two_phases(replicated, args, _World(monkeypatch)), want)         # the cached workspace
    # more ranks than items: five of eight ranks hold nothing and contribute zeros without a kernel
    few = Evaluator([sorted({i % 3 for i in m[:1]}) for m in mask], [sorted({g % 3 for g in row[:2]}) for row in gt], 3, "cuda")
    Q3 = Q[:3].contiguous()
    monkeypatch.undo()
    want3 = few.rank_positions(kind, model.user_embedding, uid, Q3, model.w, model.w_user, model.rubi_c)
    got3 = _two_phases([(few, Q3, None)] * 8, args, _World(monkeypatch))
    assert torch.equal(got3, want3) and int(want3.max()) >= 1
    # the report on top
    monkeypatch.undo()
    group_of = np.arange(N) % 6
    rep = whole.rank_report(kind, model.user_embedding, uid, Q, model.w, model.w_user, model.rubi_c, group_of=group_of, n_groups=6)
    got = whole.rank_report_sharded(kind, model.user_embedding, uid, Q, model.w, model.w_user, model.rubi_c, group_of=group_of, n_groups=6)
    assert sorted(rep) == sorted(got) and all(np.array_equal(rep[k], got[k], equal_nan=True) for k in rep)


def test_evaluator_sharded_positions_lightgcn_ego_branch(ops, monkeypatch):
    from macr_amd.evaluator import Evaluator
    rs = np.random.RandomState(22)
    n_users, N, U = 400, 2000, 300
    model = base._lgcn_model(n_users, N)
    model.update_c(None, 0.02)
    ua, ia = model.propagated()
    ia, ego = ia.contiguous(), model.ego_items()
    uid = dev(rs.permutation(n_users)[:U].astype(np.int32))
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(U)]
    gt = [sorted(rs.choice(N, rs.randint(1, 25), replace=False).tolist()) for _ in range(U)]
    want = Evaluator(mask, gt, N, "cuda").rank_positions(ops.SCORE_RUBI, ua, uid, ia, model.w, model.w_user, model.rubi_c, branch=ego)
    shards = [(Evaluator(mask, gt, N, "cuda"), ia, ego) for _ in range(2)]
    got = _two_phases(shards, (ops.SCORE_RUBI, ua, uid, model.w, model.w_user, model.rubi_c), _World(monkeypatch))
    assert torch.equal(got, want) and int(want.max()) > N // 2


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _env(**extra):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.pop("MACR_RANK_REPORT", None)
    env.pop("MACR_SHARD_RANK_REPORT", None)
    env.update(extra)
    return env


def _run(cmd, cwd, ranks=1, port=None, **extra):
    head = [sys.executable]
    if ranks > 1:
        head += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                 "--master-port", str(port)]
        extra["MACR_DIST_BACKEND"] = "gloo"            # the rig: several ranks on this GPU
    out = subprocess.run(head + cmd, cwd=cwd, env=_env(**extra), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


_rank_lines = base._rank_lines
_metric_lines = lambda out: [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if "recall=" in l]
OLD, NEW = dict(MACR_RANK_REPORT="1"), dict(MACR_SHARD_RANK_REPORT="1")


def test_mf_cli_same_line_from_one_process_two_ranks_and_row_shards(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    cmd = [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset", "tiny_data",
           "--batch_size", "16", "--cuda", "0", "--saveID", "d", "--log_interval", "1", "--lr", "0.01", "--epoch", "3", "--train",
           "rubibceboth", "--test", "rubi", "--c", "0.5", "--Ks", "[5, 20]", "--save_flag", "1", "--verbose", "1"]
    cwd = str(tmp_path)
    trained = _rank_lines(_run(cmd, cwd, **OLD))
    assert len(trained) == 3
    cmd += ["--pretrain", "1"]                             # the newest checkpoint: the last evaluation's model
    plain = _run(cmd, cwd)
    assert "rank:" not in plain and len(_metric_lines(plain)) == 1
    one = _run(cmd, cwd, **NEW)
    assert _rank_lines(one) == trained[-1:] and _metric_lines(one) == _metric_lines(plain)
    assert _rank_lines(_run(cmd, cwd, **OLD, **NEW)) == trained[-1:]              # both switches: one line
    assert _rank_lines(_run(cmd + ["--row_shard", "1"], cwd, **NEW)) == trained[-1:]
    assert _rank_lines(_run(cmd, cwd, ranks=2, port=29571, **NEW)) == trained[-1:]       # the main rank alone prints
    assert _rank_lines(_run(cmd + ["--row_shard", "1"], cwd, ranks=2, port=29573, **NEW)) == trained[-1:]


def test_lightgcn_cli_same_line_from_one_process_and_two_ranks(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    cmd = [os.path.join(REPO, "macr_lightgcn", "LightGCN.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset", "tiny_data",
           "--verbose", "1", "--layer_size", "[64,64]", "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0",
           "--epoch", "3", "--log_interval", "1", "--weights_path", str(tmp_path) + "/", "--saveID", "d", "--loss", "bce",
           "--test", "normal", "--c", "0.5"]
    cwd = str(tmp_path)
    trained = _rank_lines(_run(cmd, cwd, **NEW))           # while training, one process: a line per evaluation
    assert len(trained) == 3
    cmd += ["--pretrain", "1"]                             # the saved model at c = 0 and at --c: two evaluations
    whole = _run(cmd, cwd, **OLD)
    want = _rank_lines(whole)
    assert len(want) == 2
    plain = _run(cmd, cwd)
    assert "rank:" not in plain and _metric_lines(plain) == _metric_lines(whole) and len(_metric_lines(plain)) == 2
    assert _rank_lines(_run(cmd, cwd, **NEW)) == want
    assert _rank_lines(_run(cmd, cwd, ranks=2, port=29575, **NEW)) == want
