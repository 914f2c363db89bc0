"""The bit-reproducible row-sharded MF step on the GPU (-m gpu): HipBackend(deterministic=True) / macr_shard_*_det /
MACR_SHARD_DETERMINISTIC=1, in the in-process worlds of tests/shard_loopback.py (W threads, one GPU context, the production
RowShardedMF.step / step_split).  Problems are built as in tests/test_gpu_shard_worlds.py; the hot runs are written by hand, as
in tests/test_gpu_deterministic.py, so that reference counts are known (chunks of k_seg_reduce: 16 references, 8 at d = 32).
Every shape is the smallest that reaches a place where an order could leak:

    B300   W3  d64  range  40 x 50        150 references to the last item row (rank 2), 75 to item 1 (rank 0), 150 to a user row
                                          of the middle rank: runs of ten chunks on three different ranks, shards with lo > 0,
                                          more positions than users
    B100   W8  d32  interleaved  5 x 77   item 0 48 times: chunks of 8; ranks 5..7 own no user row; fewer row blocks than ranks
    B257   W2  d256 range  300 x 80       item 0 130 times; one lane group per wave
    B4096  W3 / W16  d64  5003 x 1201     item 0 2048 times, item 1 1024 times as negative: 256 backward blocks, 32 per
                                          branch-vector slot; a 128-chunk fold
    B100   W8  d128 split                 slices of 12 / 13 positions that begin at no block boundary
    B777   W3  d64  both layouts, lazy K = 3, seven steps with a flush after the fourth, item 0 200 times: every sweep phase, rows
                                          behind when gathered

1. repeatability: three fresh worlds per case -- losses of every step on every rank, every rank's tables and slots, w, w_user,
   their slots, adam_pow and the stamps after the flush equal BIT FOR BIT.  Whether two default-mode worlds differed on the
   same batches is put on record, not asserted.
2. collective-order independence: the same cases through Loopbacks whose all_reduce adds the ranks' tensors in reversed order,
   and in an order rotated by call count: bit-identical to the rank-order run (W >= 3, both step forms).
3. accuracy: against oracle.mf_train_step / tests/bpr_ref.py at the tolerances of tests/test_gpu_shard_worlds.py.
4. path and hygiene (asserted inside every deterministic run, tests/shard_rig.py): the kernels of the last step; gradient scratch and row flags
   clean after every step on every rank; the ranks of one run agree bit for bit on losses, w and w_user after every step.
5. product: ShardedBPRMF under the variable, and two runs of the MF CLI with --row_shard 1: bit-identical checkpoints."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import shard_loopback
import shard_rig
from helpers import GOLD, REPO
from shard_rig import ALL_FORMS, BOTH, BPR, ITEM, LR, NORMAL, SMALL, TABLES, ReversedLoopback, RotatingLoopback, bits, dev, set_form

pytestmark = pytest.mark.gpu

# name -> B, d, n_users, n_items, W, layout, lazy period, steps, flush after step, hot runs [(array, start, stop, row)]
SHAPES = {
    "B300": (300, 64, 40, 50, 3, "range", 1, 3, None, (("i", 0, 150, 49), ("j", 150, 225, 1), ("u", 0, 150, 20))),
    "B100": (100, 32, 5, 77, 8, "interleaved", 1, 3, None, (("i", 0, 48, 0),)),
    "B257": (257, 256, 300, 80, 2, "range", 1, 3, None, (("i", 0, 130, 0),)),
    "B4096W3": (4096, 64, 5003, 1201, 3, "interleaved", 1, 3, None, (("i", 0, 2048, 0), ("j", 2048, 3072, 1))),
    "B4096W16": (4096, 64, 5003, 1201, 16, "interleaved", 1, 3, None, (("i", 0, 2048, 0), ("j", 2048, 3072, 1))),
    "B100d128": (100, 128, 901, 350, 8, "interleaved", 1, 3, None, (("i", 0, 40, 0),)),
    "B777i": (777, 64, 901, 350, 3, "interleaved", 3, 7, 4, (("i", 0, 200, 0),)),
    "B777r": (777, 64, 901, 350, 3, "range", 3, 7, 4, (("i", 0, 200, 0),)),
}
CASES = ([("B300", k, s) for k, s in ALL_FORMS] + [("B100", k, s) for k, s in ALL_FORMS] + [("B257", k, s) for k, s in ALL_FORMS] +
         [(sh, BOTH, s) for sh in ("B4096W3", "B4096W16") for s in (True, False)] +
         [("B100d128", BOTH, True), ("B100d128", ITEM, True)] +
         [("B777i", BOTH, True), ("B777i", BOTH, False), ("B777i", BPR, False)] +
         [("B777r", BOTH, True), ("B777r", ITEM, False), ("B777r", NORMAL, False)])


def case_id(c):
    return "%s-%s-%s" % (c[0], c[1][5:].lower(), "split" if c[2] else "replicated")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def spec_of(shape):
    """(problem, case without its kind and form) of a shape, as shard_rig.run_world takes them"""
    B, d, n_users, n_items, W, layout, lazy, steps, flush_after, hot = SHAPES[shape]
    return (B, d, n_users, n_items, steps, flush_after, hot), (W, layout, lazy)


def problem_of(shape):
    B, d, n_users, n_items, steps, flush_after, hot = spec_of(shape)[0]
    return shard_rig.problem(B, d, n_users, n_items, steps, hot)


def run_world(ops, case, deterministic, loopback=None):
    """the case's steps on its W ranks -> per rank: what it saw after every step and its shard at the end (numpy); the
    deterministic runs assert their path and hygiene inside (shard_rig.run_world)"""
    shape, kind_name, split = case
    spec, where = spec_of(shape)
    return shard_rig.run_world(ops, spec, (kind_name, split) + where, "det" if deterministic else "plain", loopback)["ranks"]


def differences(x, y):
    """names of what two runs of a case disagree on, rank by rank"""
    out = []
    for rank, (a, b) in enumerate(zip(x, y)):
        for name in ("losses", "w", "wu"):
            out += ["rank %d %s step %d" % (rank, name, k) for k in range(len(a[name])) if not bits(a[name][k], b[name][k])]
        for name in TABLES + SMALL + ("adam_pow", "m1P", "m1Q") + (("stP", "stQ") if "stP" in a else ()):
            if not bits(a[name], b[name]):
                out.append("rank %d %s" % (rank, name))
    return out


_first = {}


def first_run(ops, case):
    """the rank-order deterministic run of a case, once (tests 1 - 3 share it and leave it unchanged)"""
    if case not in _first:
        _first[case] = run_world(ops, case, True)
    return _first[case]


# ----------------------------------------------------------------------------- 1. repeatability
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fresh_worlds_agree_bit_for_bit(ops, monkeypatch, record_property, case):
    set_form(monkeypatch, case[2])
    shape = case[0]
    B, d, n_users, n_items, W, layout = SHAPES[shape][:6]
    if shape == "B300":                                 # the hot rows lie where the table says
        from macr_amd import sharded_train
        own_u, own_i = sharded_train.Owned(n_users, 0, W, layout), sharded_train.Owned(n_items, 0, W, layout)
        assert int(own_i.owner_of(torch.tensor([49]))) == 2 and int(own_i.owner_of(torch.tensor([1]))) == 0
        assert int(own_u.owner_of(torch.tensor([20]))) == 1
    a = first_run(ops, case)
    for other in (run_world(ops, case, True), run_world(ops, case, True)):
        assert differences(a, other) == []
    assert not bits(a[0]["P"], torch.from_numpy(np.array(problem_of(shape)[0]))[a[0]["own_u"].global_ids()])       # (it trained)
    x, y = run_world(ops, case, False), run_world(ops, case, False)
    diff = differences(x, y)
    record_property("default_mode_worlds_differed", bool(diff))
    print("%s: two default-mode worlds differed: %s %s" % (case_id(case), bool(diff), diff[:4]))


# ----------------------------------------------------------------------------- 2. collective-order independence
@pytest.mark.parametrize("case", [c for c in CASES if SHAPES[c[0]][4] >= 3], ids=case_id)
def test_result_does_not_depend_on_the_order_a_collective_adds_in(ops, monkeypatch, case):
    set_form(monkeypatch, case[2])
    a = first_run(ops, case)
    for loopback in (ReversedLoopback, RotatingLoopback):
        assert differences(a, run_world(ops, case, True, loopback)) == [], loopback.__name__


# ----------------------------------------------------------------------------- 3. accuracy
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_the_cpu_restatements(ops, monkeypatch, record_property, case):
    set_form(monkeypatch, case[2])
    shape, kind_name, split = case
    B, d, n_users, n_items, W, layout, lazy, steps, flush_after, hot = SHAPES[shape]
    ranks = first_run(ops, case)
    want_losses, want_m1, Po, Qo, wo, wuo = shard_rig.cpu_reference(B, d, n_users, n_items, steps, hot, kind_name)
    full = {}
    for name in ("P", "m1P"):
        full[name] = shard_loopback.reassemble([r[name] for r in ranks], [r["own_u"] for r in ranks], n_users).numpy()
    for name in ("Q", "m1Q"):
        full[name] = shard_loopback.reassemble([r[name] for r in ranks], [r["own_i"] for r in ranks], n_items).numpy()
    tol = 2e-3 * LR * steps
    worst_loss = max(float(np.abs(got / want - 1).max()) for r in ranks for got, want in zip(r["losses"], want_losses))
    worst_tab = max(float(np.abs(full["P"] - Po).max()), float(np.abs(full["Q"] - Qo).max()),
                    max(float(np.abs(r["w"][-1] - wo).max()) for r in ranks), max(float(np.abs(r["wu"][-1] - wuo).max()) for r in ranks))
    record_property("worst_loss_rel", worst_loss)
    record_property("worst_table_abs", worst_tab)
    print("%s: worst loss rel %.3g (1e-5), worst table abs %.3g (%.3g)" % (case_id(case), worst_loss, worst_tab, tol))
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


# ----------------------------------------------------------------------------- 4. the fold kernel itself
def test_fold_ranks_adds_the_rows_in_rank_order(ops):
    from macr_amd import _lib
    rs = np.random.RandomState(5)
    for world, n in ((1, 7), (3, 1000), (16, 70001)):
        parts = (rs.standard_normal((world, n)) * 10.0 ** rs.randint(-6, 6, (world, n))).astype(np.float32)
        want = parts[0].copy()
        for r in range(1, world):
            want = want + parts[r]                      # fp32, rank order
        t, out = dev(parts), torch.full((n,), 7.0, device="cuda")
        _lib.check(_lib.lib().macr_shard_fold_ranks(world, n, ops._ptr(t), ops._ptr(out), ops._stream()))
        assert bits(out.cpu(), want), (world, n)


# ----------------------------------------------------------------------------- 5. product
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=300, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


@pytest.mark.parametrize("train", ["rubibceboth", "rubibce", "normalbce", "normal"])
def test_model_under_the_variable_trains_bit_identically(ops, train, monkeypatch):
    from macr_amd.mf import ShardedBPRMF
    monkeypatch.setenv("MACR_SHARD_DETERMINISTIC", "1")
    cfg = dict(n_users=40, n_items=50)
    a, b = ShardedBPRMF(_mf_args(), cfg, seed=7), ShardedBPRMF(_mf_args(), cfg, seed=7)
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")                          # both switches: the sharded one decides
    assert ShardedBPRMF(_mf_args(), cfg, seed=7).deterministic
    monkeypatch.delenv("MACR_DETERMINISTIC")
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC")
    off = ShardedBPRMF(_mf_args(), cfg, seed=7)
    assert a.deterministic and b.deterministic and not off.deterministic
    assert ShardedBPRMF(_mf_args(), cfg, seed=7, deterministic=True).deterministic          # the keyword, without the variable
    kind = a.kind_of(train)
    for u, i, j in problem_of("B300")[4]:                                  # hot-row batches: 40 users, 50 items
        for m in (a, b, off):
            m.train_step(kind, m.to_device_batch(u.tolist(), i.tolist(), j.tolist()))
    assert all(m._model(kind).deterministic and m._model(kind).backend.deterministic for m in (a, b))
    assert not off._model(kind).deterministic
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and "opt%d.adam_pow" % kind in sa
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert bits(sa[k].cpu(), sb[k].cpu()), k
        else:
            assert sa[k] == sb[k], k
    so = off.state_dict()
    assert float((sa["user_embedding"] - so["user_embedding"]).abs().max()) <= 2e-3 * 1e-3 * 3     # rounding apart, no more


def test_mf_cli_row_sharded_runs_are_bit_identical(ops, tmp_path):
    """one process is the smallest world the CLI accepts with --row_shard 1"""
    outs, ckpts = [], []
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
        shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / name / "data" / "tiny_data")
        env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_SHARD_DETERMINISTIC="1")
        for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MACR_DETERMINISTIC"):
            env.pop(v, None)
        cmd = [sys.executable, os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / name / "data") + "/",
               "--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0", "--saveID", "sdet", "--log_interval", "1", "--lr", "0.01",
               "--epoch", "4", "--train", "rubibceboth", "--test", "rubi", "--c", "40", "--Ks", "[5]", "--save_flag", "1",
               "--row_shard", "1"]
        out = subprocess.run(cmd, cwd=str(tmp_path / name), env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        found = {}
        for root, _, files in os.walk(str(tmp_path / name)):
            for f in files:
                if f.endswith("_ckpt.pt"):
                    found[f] = torch.load(os.path.join(root, f), map_location="cpu")
        outs.append(out.stdout)
        ckpts.append(found)
    ck_a, ck_b = ckpts
    assert sorted(ck_a) == sorted(ck_b) == ["%d_ckpt.pt" % e for e in range(4)], (sorted(ck_a), sorted(ck_b))
    for f in ck_a:
        assert sorted(ck_a[f]) == sorted(ck_b[f])
        for k, v in ck_a[f].items():
            if torch.is_tensor(v):
                assert bits(v, ck_b[f][k]), (f, k)
            else:
                assert v == ck_b[f][k], (f, k)
    assert not torch.equal(ck_a["0_ckpt.pt"]["user_embedding"], ck_a["3_ckpt.pt"]["user_embedding"])
    train = lambda out: [l.split("train==[")[1].split("]")[0] for l in out.splitlines() if "train==[" in l]
    ta, tb = train(outs[0]), train(outs[1])
    assert len(ta) == 4 and ta == tb, (ta, tb)


def test_mf_cli_refuses_the_variable_without_row_shard(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_SHARD_DETERMINISTIC="1")
    cmd = [sys.executable, os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset",
           "tiny_data", "--batch_size", "16", "--cuda", "0", "--epoch", "1", "--train", "rubibceboth", "--test", "rubi"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "MACR_DETERMINISTIC" in out.stderr and "--row_shard 1" in out.stderr, out.stderr[-2000:]
