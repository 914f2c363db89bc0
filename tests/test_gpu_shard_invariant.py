"""The rank-count-invariant row-sharded MF step on the GPU (-m gpu): HipBackend(invariant=True) / macr_shard_*_inv /
MACR_SHARD_INVARIANT=1, in the in-process worlds of tests/shard_loopback.py (W threads, one GPU context, the production
RowShardedMF.step / step_split).  Problems are built as in tests/test_gpu_shard_deterministic.py; the hot runs are written by
hand, so that the same run lies at different offsets of the rank-local sorted reference list for different W and layouts
(chunks of the row sums: 16 references, 8 at d = 32).  The reference of a problem is the new mode at WORLD 1 (replicated step,
dense pass).

    P300   B=300  d=64  40 x 50       W 2, 3, 5 x range, interleaved: 150 references to item 49, 75 to item 1, 150 to user 20
                                      -- runs of ten chunks that start mid-window on some ranks
    P100   B=100  d=32  5 x 77        W 3, 8, 16: item 0 48 times; chunks of 8; ranks without user rows; fewer row blocks than
                                      ranks; empty slices under the 32-aligned rule (4 aligned blocks on 8 and 16 ranks)
    P257   B=257  d=256 300 x 80      W 2, 3: item 0 130 times; one lane group per wave; a last block of one position
    P4096  B=4096 d=64  5003 x 1201   W 3, 16: item 0 2048 times, item 1 1024 times; 256 backward blocks; a 128-chunk fold
    P100d  B=100  d=128               W 8, split: slices under the new rule
    P777   B=777  d=64  seven steps   W 3, both layouts, lazy K 2 and 3 against K = 1 at world 1, a flush after step 4
    P16416 B=16416 d=256              W 2: more than 4096 backward blocks -- the split form is refused, the step takes the
                                      replicated form (invariance only: the CPU restatement of a 16416 x 16416 term is no quick test)

1. invariance: every world, layout, form and period equals the world-1 reference BIT FOR BIT on the losses of every step on every
   rank, the reassembled tables and slots after the flushes, w, w_user (every step), their slots and adam_pow.
2. repeatability and collective-order independence: a fresh world, and (W >= 3) Loopbacks that add in reversed and in
   call-rotated order, are bit-identical to the first run.
3. accuracy: against oracle.mf_train_step / tests/bpr_ref.py at the tolerances of tests/test_gpu_shard_worlds.py.
4. path and hygiene (asserted inside every run): the kernels of the last step are the new ones; gradient scratch and row flags
   clean after every step on every rank.
5. on record, not asserted: whether MACR_SHARD_DETERMINISTIC worlds differed from their own world 1 on the same problems.
6. product: ShardedBPRMF under the variable; the MF CLI as one process and as two ranks: identical losses and checkpoints."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import shard_rig
from helpers import GOLD, REPO
from shard_rig import (ALL_FORMS, BOTH, ITEM, LR, DECAY, ALPHA, BETA, BS, SMALL, TABLES, ReversedLoopback, RotatingLoopback, bits,
                       set_form)

pytestmark = pytest.mark.gpu

# name -> B, d, n_users, n_items, steps, flush after step, hot runs [(array, start, stop, row)]
PROBLEMS = {
    "P300": (300, 64, 40, 50, 3, None, (("i", 0, 150, 49), ("j", 150, 225, 1), ("u", 0, 150, 20))),
    "P100": (100, 32, 5, 77, 3, None, (("i", 0, 48, 0),)),
    "P257": (257, 256, 300, 80, 3, None, (("i", 0, 130, 0),)),
    "P4096": (4096, 64, 5003, 1201, 3, None, (("i", 0, 2048, 0), ("j", 2048, 3072, 1))),
    "P100d": (100, 128, 901, 350, 3, None, (("i", 0, 40, 0),)),
    "P777": (777, 64, 901, 350, 7, 4, (("i", 0, 200, 0),)),
    "P16416": (16416, 256, 300, 80, 2, None, (("i", 0, 130, 0),)),      # 4104 backward blocks: beyond the split form's 4096
}
# a case: (problem, kind, split, W, layout, lazy period)
CASES = ([("P300", k, s, W, lay, 1) for k, s in ALL_FORMS for W in (2, 3, 5) for lay in ("range", "interleaved")] +
         [("P100", k, s, W, "interleaved", 1) for k, s in ALL_FORMS for W in (3, 8, 16)] +
         [("P257", k, s, W, "range", 1) for k, s in ALL_FORMS for W in (2, 3)] +
         [("P4096", BOTH, s, W, "interleaved", 1) for s in (True, False) for W in (3, 16)] +
         [("P100d", BOTH, True, 8, "interleaved", 1), ("P100d", ITEM, True, 8, "interleaved", 1)] +
         [("P777", BOTH, s, 3, lay, K) for s in (True, False) for lay in ("range", "interleaved") for K in (2, 3)])


def case_id(c):
    return "%s-%s-%s-W%d-%s-K%d" % (c[0], c[1][5:].lower(), "split" if c[2] else "replicated", c[3], c[4], c[5])


def reference_case(c):
    """world 1, replicated, dense pass: what every case of (problem, kind) must equal"""
    return (c[0], c[1], False, 1, "interleaved", 1)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def problem(name):
    B, d, n_users, n_items, steps, flush_after, hot = PROBLEMS[name]
    return shard_rig.problem(B, d, n_users, n_items, steps, hot)


def cpu_reference(name, kind_name):
    B, d, n_users, n_items, steps, flush_after, hot = PROBLEMS[name]
    return shard_rig.cpu_reference(B, d, n_users, n_items, steps, hot, kind_name)


def run_world(ops, case, mode="inv", loopback=None):
    """the case's steps on its W ranks -> what the contract speaks of: losses, w, w_user after every step per rank; the
    reassembled tables and slots after every flush; the branch slots and adam_pow at the end (shard_rig.run_world, which asserts
    the mode's path and hygiene inside)"""
    return shard_rig.run_world(ops, PROBLEMS[case[0]], case[1:], mode, loopback)


def differences(x, ref):
    """names of what a world disagrees on with a reference world (of any number of ranks): every rank of x against rank 0 of ref
    for what every rank holds, the reassembled tables for what is sharded"""
    out, r0 = [], ref["ranks"][0]
    for rank, a in enumerate(x["ranks"]):
        for name in ("losses", "w", "wu"):
            out += ["rank %d %s step %d" % (rank, name, k) for k in range(len(r0[name])) if not bits(a[name][k], r0[name][k])]
        out += ["rank %d %s" % (rank, name) for name in SMALL + ("adam_pow",) if not bits(a[name], r0[name])]
    assert len(x["full"]) == len(ref["full"])
    for f, (a, b) in enumerate(zip(x["full"], ref["full"])):
        out += ["%s after flush %d" % (t, f) for t in TABLES if not bits(a[t], b[t])]
    return out


_first = {}


def first_run(ops, case, mode="inv"):
    """the rank-order run of a case, once (the tests share it and leave it unchanged)"""
    if (case, mode) not in _first:
        _first[(case, mode)] = run_world(ops, case, mode)
    return _first[(case, mode)]


def world_one(ops, monkeypatch, case, mode="inv"):
    set_form(monkeypatch, False)
    return first_run(ops, reference_case(case), mode)


# ----------------------------------------------------------------------------- 1. invariance
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_world_equals_world_one_bit_for_bit(ops, monkeypatch, case):
    ref = world_one(ops, monkeypatch, case)
    set_form(monkeypatch, case[2])
    name, W, layout = case[0], case[3], case[4]
    if name == "P300" and W == 3 and layout == "range":              # the hot rows lie on three different ranks
        from macr_amd import sharded_train
        own_u, own_i = sharded_train.Owned(40, 0, 3, layout), sharded_train.Owned(50, 0, 3, layout)
        assert int(own_i.owner_of(torch.tensor([49]))) == 2 and int(own_i.owner_of(torch.tensor([1]))) == 0
        assert int(own_u.owner_of(torch.tensor([20]))) == 1
    if case[2]:                                                      # the split form runs on slices of the new rule
        from macr_amd import _lib, sharded_train
        be = sharded_train.HipBackend(getattr(ops, case[1]), PROBLEMS[name][1], ops.make_hyper(LR, DECAY, ALPHA, BETA, BS),
                                      torch.device("cuda"), invariant=True)
        cuts = [be.slice_of(PROBLEMS[name][0], r, W) for r in range(W)]
        assert all(t0 % 32 == 0 for t0, _ in cuts) and cuts[-1][1] == PROBLEMS[name][0]
        if name == "P100" and W >= 8:
            assert any(t0 == t1 for t0, t1 in cuts)                  # empty slices
    got = first_run(ops, case)
    assert differences(got, ref) == []
    P0 = torch.from_numpy(np.array(problem(name)[0]))
    assert not bits(got["full"][-1]["P"], P0)                        # (it trained)


def test_a_batch_beyond_4096_blocks_takes_the_replicated_form(ops, monkeypatch):
    from macr_amd import _lib, sharded_train
    case = ("P16416", BOTH, True, 2, "interleaved", 1)
    be = sharded_train.HipBackend(ops.LOSS_RUBIBCEBOTH, 256, ops.make_hyper(LR, DECAY, ALPHA, BETA, BS), torch.device("cuda"),
                                  invariant=True)
    assert be.slice_of(16384, 1, 2) == (8192, 16384)
    with pytest.raises(_lib.MacrError) as e:
        be.slice_of(16416, 0, 2)
    assert e.value.code == _lib.E_UNSUPPORTED
    ref = world_one(ops, monkeypatch, case)
    set_form(monkeypatch, True)                                      # the split form is asked for ...
    got = first_run(ops, case)
    assert differences(got, ref) == []
    kernels = got["ranks"][0]["kernels"]                             # ... and the replicated one ran
    assert "shard_gather" in kernels and not kernels & {"shard_route"}, kernels


# ----------------------------------------------------------------------------- 2. repeatability, collective-order independence
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fresh_worlds_and_other_collective_orders_agree(ops, monkeypatch, case):
    set_form(monkeypatch, case[2])
    a = first_run(ops, case)
    assert differences(run_world(ops, case), a) == []
    if case[3] >= 3:
        for loopback in (ReversedLoopback, RotatingLoopback):
            assert differences(run_world(ops, case, "inv", loopback), a) == [], loopback.__name__


# ----------------------------------------------------------------------------- 3. accuracy
@pytest.mark.parametrize("case", CASES + sorted({reference_case(c) for c in CASES}), ids=case_id)
def test_against_the_cpu_restatements(ops, monkeypatch, record_property, case):
    set_form(monkeypatch, case[2])
    name, kind_name = case[0], case[1]
    steps = PROBLEMS[name][4]
    world = first_run(ops, case)
    ranks = world["ranks"]
    want_losses, want_m1, Po, Qo, wo, wuo = cpu_reference(name, kind_name)
    last = world["full"][-1]
    tol = 2e-3 * LR * steps
    worst_loss = max(float(np.abs(got / want - 1).max()) for r in ranks for got, want in zip(r["losses"], want_losses))
    worst_tab = max(float(np.abs(last["P"].numpy() - Po).max()), float(np.abs(last["Q"].numpy() - Qo).max()),
                    max(float(np.abs(r["w"][-1] - wo).max()) for r in ranks), max(float(np.abs(r["wu"][-1] - wuo).max()) for r in ranks))
    record_property("worst_loss_rel", worst_loss)
    record_property("worst_table_abs", worst_tab)
    print("%s: worst loss rel %.3g (1e-5), worst table abs %.3g (%.3g)" % (case_id(case), worst_loss, worst_tab, tol))
    for r in ranks:                                                         # losses on EVERY rank
        for got, want in zip(r["losses"], want_losses):
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    for tname, got, want in (("mP", world["m1P"].numpy(), want_m1[0]), ("mQ", world["m1Q"].numpy(), want_m1[1])):
        np.testing.assert_allclose(got / 0.1, want / 0.1, rtol=2e-4, atol=2e-6 * np.abs(want / 0.1).max(), err_msg=tname)
    for tname, got, want in (("P", last["P"].numpy(), Po), ("Q", last["Q"].numpy(), Qo)):
        np.testing.assert_allclose(got, want, rtol=0, atol=tol, err_msg=tname)
    for r in ranks:
        np.testing.assert_allclose(r["w"][-1], wo, rtol=0, atol=tol)
        np.testing.assert_allclose(r["wu"][-1], wuo, rtol=0, atol=tol)


# ----------------------------------------------------------------------------- 5. on record: the deterministic mode across worlds
RECORD = [c for c in CASES if c[1] == BOTH and (c[0] != "P300" or c[3] == 3)]


@pytest.mark.parametrize("case", RECORD, ids=case_id)
def test_record_whether_deterministic_worlds_differ_from_their_world_one(ops, monkeypatch, record_property, case):
    ref = world_one(ops, monkeypatch, case, "det")
    set_form(monkeypatch, case[2])
    diff = differences(run_world(ops, case, "det"), ref)
    record_property("deterministic_world_differed_from_world_one", bool(diff))
    print("%s: MACR_SHARD_DETERMINISTIC world differed from its world 1: %s %s" % (case_id(case), bool(diff), diff[:4]))


# ----------------------------------------------------------------------------- 6. product
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=300, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


@pytest.mark.parametrize("train", ["rubibceboth", "rubibce", "normalbce", "normal"])
def test_model_under_the_variable_carries_the_mode(ops, train, monkeypatch):
    from macr_amd.mf import ShardedBPRMF
    for name in ("MACR_SHARD_DETERMINISTIC", "MACR_DETERMINISTIC"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MACR_SHARD_INVARIANT", "1")
    cfg = dict(n_users=40, n_items=50)
    a, b = ShardedBPRMF(_mf_args(), cfg, seed=7), ShardedBPRMF(_mf_args(), cfg, seed=7)
    monkeypatch.setenv("MACR_SHARD_DETERMINISTIC", "1")                    # both switches: the invariant one wins
    both = ShardedBPRMF(_mf_args(), cfg, seed=7)
    assert both.invariant and both._model(both.kind_of(train)).invariant and not both._model(both.kind_of(train)).deterministic
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC")
    monkeypatch.delenv("MACR_SHARD_INVARIANT")
    off = ShardedBPRMF(_mf_args(), cfg, seed=7)
    assert a.invariant and b.invariant and not off.invariant
    assert ShardedBPRMF(_mf_args(), cfg, seed=7, invariant=True).invariant                  # the keyword, without the variable
    kind = a.kind_of(train)
    ops.timing_begin()
    for u, i, j in problem("P300")[4]:                                     # hot-row batches: 40 users, 50 items
        for m in (a, b, off):
            m.train_step(kind, m.to_device_batch(u.tolist(), i.tolist(), j.tolist()))
    kernels = {n for n, _ in ops.timing_end(250)}
    assert "seg_reduce_inv" in kernels and "seg_fold_inv" in kernels, kernels
    assert all(m._model(kind).invariant and m._model(kind).backend.invariant for m in (a, b))
    assert not off._model(kind).invariant
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and "opt%d.adam_pow" % kind in sa
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert bits(sa[k].cpu(), sb[k].cpu()), k
        else:
            assert sa[k] == sb[k], k
    so = off.state_dict()
    assert float((sa["user_embedding"] - so["user_embedding"]).abs().max()) <= 2e-3 * 1e-3 * 3     # rounding apart, no more


def test_mf_cli_one_process_and_two_ranks_are_bit_identical(ops, tmp_path):
    """--row_shard 1 under the variable, once as a single process and once as two ranks (gloo rig, both ranks on this GPU): the
    same train==[..] columns and bit-identical checkpoint tensors (rank 0 writes the reassembled tables)"""
    outs, ckpts = [], []
    cli = [os.path.join(REPO, "macr_mf", "train.py")]
    for name, launcher in (("one", [sys.executable]),
                           ("two", [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                                    "--master-addr", "127.0.0.1", "--master-port", "29561"])):
        (tmp_path / name).mkdir()
        shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / name / "data" / "tiny_data")
        env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_SHARD_INVARIANT="1", MACR_DIST_BACKEND="gloo")
        for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MACR_DETERMINISTIC", "MACR_SHARD_DETERMINISTIC", "MACR_SHARD_SPLIT",
                  "MACR_LAZY_ADAM"):
            env.pop(v, None)
        cmd = launcher + cli + ["--data_path", str(tmp_path / name / "data") + "/", "--dataset", "tiny_data", "--batch_size", "16",
                                "--cuda", "0", "--saveID", "sinv", "--log_interval", "1", "--lr", "0.01", "--epoch", "4", "--train",
                                "rubibceboth", "--test", "rubi", "--c", "40", "--Ks", "[5]", "--save_flag", "1", "--row_shard", "1"]
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
    env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_SHARD_INVARIANT="1")
    env.pop("MACR_SHARD_DETERMINISTIC", None)
    cmd = [sys.executable, os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset",
           "tiny_data", "--batch_size", "16", "--cuda", "0", "--epoch", "1", "--train", "rubibceboth", "--test", "rubi"]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "MACR_SHARD_INVARIANT" in out.stderr and "--row_shard 1" in out.stderr, out.stderr[-2000:]
