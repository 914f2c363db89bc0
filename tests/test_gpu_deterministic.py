"""The bit-reproducible MF step on the GPU (-m gpu): MFState(deterministic=True) / MACR_STEP_DETERMINISTIC / MACR_DETERMINISTIC=1.

The problems are those of tests/mf_det_cases.py (its docstring lists the shapes and what each one reaches).

1. repeatability: three fresh deterministic states, six steps on the same batches, complete steps and (the (B,B) kinds) a
   deferred sequence ended by flush(): losses of every step, P, Q, w, wu, the eight slots and adam_pow equal BIT FOR BIT.
   Whether two default-mode states differed on the same batches is put on record, not asserted.
2. accuracy: the same trajectories against the CPU restatements (oracle.mf_train_step for the BCE kinds, tests/bpr_ref.py for
   `normal`, tests/rubi_bpr_ref.py for `rubi`) at the tolerances of tests/test_gpu_bpr.py / tests/test_gpu_shard_worlds.py.
3. hygiene: one step from equal states, deterministic against default, as test_row_shard_world1_bpr_equals_unsharded_step
   requires of two routes; gradient scratch and row flags zero after every deterministic step.
4. the model under MACR_DETERMINISTIC=1 and two runs of the MF CLI: bit-identical checkpoints."""
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
import oracle
import rubi_bpr_ref
from helpers import GOLD, REPO
from mf_det_cases import (ALPHA, BETA, BS, BXB_KINDS, DECAY, KINDS, LR, SHAPES, STATE_NAMES, STEPS, assert_clean, bits_equal,
                          device_batches, fresh, problem, run)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


# ----------------------------------------------------------------------------- 1. repeatability
@pytest.mark.parametrize("kind_name", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_deterministic_runs_are_bit_identical(ops, shape, kind_name, record_property):
    modes = [False] + ([True] if kind_name in BXB_KINDS else [])
    for defer in modes:
        runs = [run(ops, shape, kind_name, True, defer=defer) for _ in range(3)]
        l0, s0 = runs[0]
        assert bool(torch.isfinite(l0).all()), l0
        for k, (l, s) in enumerate(runs[1:], 1):
            assert bits_equal(l, l0), ("losses", defer, k, l, l0)
            for n in STATE_NAMES:
                assert bits_equal(s[n], s0[n]), (n, defer, k, float((s[n] - s0[n]).abs().max()))
    # the default step on the same batches: on record, not asserted (its atomics' order is the hardware's)
    (la, sa), (lb, sb) = run(ops, shape, kind_name, False), run(ops, shape, kind_name, False)
    differed = sorted(n for n in STATE_NAMES if not bits_equal(sa[n], sb[n])) + ([] if bits_equal(la, lb) else ["losses"])
    record_property("default_mode_bits_differed", bool(differed))
    record_property("default_mode_differing", ",".join(differed))
    print("%s %s: default mode differed in %s" % (shape, kind_name, differed or "nothing"))


# ----------------------------------------------------------------------------- 2. accuracy
@functools.lru_cache(maxsize=None)
def reference(shape, kind_name):
    """the CPU trajectory of a problem, once: losses per step, (dP, dQ, dw, dwu) of the first step as m / 0.1, final P, Q, w, wu"""
    P, Q, w, wu, batches = problem(shape)
    d = P.shape[1]
    if kind_name in ("LOSS_BPR", "LOSS_RUBIBPR"):
        rubi = kind_name == "LOSS_RUBIBPR"
        ref = bpr_ref.Adam([P, Q, w] if rubi else [P, Q], LR)
        big = "cuda" if rubi and len(batches[0][0]) >= 4096 else None      # (the float64 (B,B) slabs on the device, as the large
        losses, m1 = [], None                                               #  cases of tests/test_gpu_rubi_bpr.py)
        for u, i, j in batches:
            if rubi:
                out = rubi_bpr_ref.mf_rubi_bpr(ref.params[0], ref.params[1], ref.params[2], u, i, j, ALPHA, DECAY, BS, device=big)
            else:
                out = bpr_ref.mf_bpr(ref.params[0], ref.params[1], u, i, j, DECAY, BS)
            ref.step(out[3:])
            losses.append(np.asarray(out[:3]))
            if m1 is None:
                m1 = [m.copy() / 0.1 for m in ref.m] + [None] * (4 - len(ref.m))
        return losses, m1, ref.params[0], ref.params[1], (ref.params[2] if rubi else w), wu
    Po, Qo, wo, wuo = P.copy(), Q.copy(), w.copy(), wu.copy()
    st = oracle.AdamState([P.shape, Q.shape, (d,), (d,)])
    losses, m1 = [], None
    for u, i, j in batches:
        losses.append(oracle.mf_train_step(getattr(oracle, kind_name), u, i, j, Po, Qo, wo, wuo, st, LR, DECAY, ALPHA, BETA, BS).copy())
        if m1 is None:
            m1 = [st.m[0] / 0.1, st.m[1] / 0.1, st.m[2] / 0.1 if kind_name != "LOSS_NORMALBCE" else None,
                  st.m[3] / 0.1 if kind_name == "LOSS_RUBIBCEBOTH" else None]
    return losses, m1, Po, Qo, wo, wuo


@pytest.mark.parametrize("kind_name", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_deterministic_trajectory_matches_the_cpu_restatement(ops, shape, kind_name):
    want_losses, m1, Pw, Qw, ww, wuw = reference(shape, kind_name)
    first = {}
    losses, s = run(ops, shape, kind_name, True, first=first)
    losses = losses.cpu().numpy()
    for t in range(STEPS):
        print("%s %s step %d: got %r want %r" % (shape, kind_name, t, losses[t].tolist(), np.asarray(want_losses[t]).tolist()))
        np.testing.assert_allclose(losses[t], want_losses[t], rtol=1e-5, err_msg="step %d" % t)
    for name, got, want in (("dP", first["mP"], m1[0]), ("dQ", first["mQ"], m1[1]), ("dw", first["mw"], m1[2]), ("dwu", first["mwu"], m1[3])):
        got = got.cpu().numpy() / 0.1
        if want is None:                                   # a vector this loss does not train
            assert not got.any(), name
            continue
        print("%s %s %s: max |err| %.3g of max %.3g" % (shape, kind_name, name, np.abs(got - want).max(), np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-6 * np.abs(want).max(), err_msg=name)
    for name, want in (("P", Pw), ("Q", Qw), ("w", ww), ("wu", wuw)):
        diff = np.abs(s[name].cpu().numpy() - want)
        print("%s %s %s: max %.3g mean %.3g (bounds %.3g, %.3g)" % (shape, kind_name, name, diff.max(), diff.mean(),
                                                                   2e-3 * LR * STEPS, 1e-4 * LR * STEPS))
        assert diff.max() <= 2e-3 * LR * STEPS and diff.mean() <= 1e-4 * LR * STEPS, (name, diff.max(), diff.mean())


# ----------------------------------------------------------------------------- 3. hygiene
@pytest.mark.parametrize("kind_name", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_deterministic_step_agrees_with_the_default_step(ops, shape, kind_name):
    kind = getattr(ops, kind_name)
    det, plain = fresh(ops, shape, True), fresh(ops, shape, False)
    u, i, j = device_batches(shape)[0]
    ops.timing_begin()
    a = det.step(kind, u, i, j).cpu().numpy()
    kernels = {n for n, _ in ops.timing_end(64)}
    b = plain.step(kind, u, i, j).cpu().numpy()
    # the staged, unfused route at every B: one owner per row, the ordered second level, the fold of the branch-vector rows
    assert {"seg_reduce", "seg_fold", "adam_dense"} <= kernels and "adam_indexed" not in kernels and "seg_sum" not in kernels, kernels
    assert ("branch_fold" in kernels) == (kind_name in BXB_KINDS), kernels
    np.testing.assert_allclose(a, b, rtol=1e-6)
    for name in ("P", "Q", "mP", "mQ"):
        x, y = getattr(det, name).cpu().numpy(), getattr(plain, name).cpu().numpy()
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6 * np.abs(y).max(), err_msg=name)
    assert_clean(det, (shape, kind_name))
    assert torch.equal(det.adam_pow, plain.adam_pow)


def test_staging_switch_does_not_leave_the_deterministic_route(ops):
    """MACR_STAGING=0 forces the default step onto its small-batch atomic path; the deterministic step stays staged (a
    subprocess: the library reads the variable once)"""
    code = ("import sys\n"
            "sys.path.insert(0, %r)\n"
            "import torch, numpy as np\n"
            "from macr_amd import ops\n"
            "rs = np.random.RandomState(0)\n"
            "t = lambda a: torch.from_numpy(a).cuda()\n"
            "P, Q = (rs.standard_normal((40, 64)) * .3).astype(np.float32), (rs.standard_normal((50, 64)) * .3).astype(np.float32)\n"
            "w = (rs.standard_normal(64) * .3).astype(np.float32)\n"
            "u, i, j = (t(rs.randint(0, n, 300).astype(np.int32)) for n in (40, 50, 50))\n"
            "i[:150] = 0\n"
            "out = []\n"
            "for _ in range(2):\n"
            "    s = ops.MFState(t(P), t(Q), t(w), t(w), ops.make_hyper(1e-3, 1e-5, 1e-2, 1e-3, 1024), 300, deterministic=True)\n"
            "    ops.timing_begin()\n"
            "    l = s.step(ops.LOSS_RUBIBCEBOTH, u, i, j).clone()\n"
            "    names = {n for n, _ in ops.timing_end(64)}\n"
            "    assert 'seg_fold' in names and 'branch_fold' in names, names\n"
            "    out.append((l, s.mQ.clone(), s.mw.clone()))\n"
            "assert all(torch.equal(a, b) for a, b in zip(*out))\n"
            "print('staged ok')\n") % REPO
    env = dict(os.environ, MACR_STAGING="0")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "staged ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# ----------------------------------------------------------------------------- 4. model and CLI
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=300, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


@pytest.mark.parametrize("train", ["rubibceboth", "rubibce", "rubi", "normalbce", "normal"])
def test_models_under_the_variable_train_bit_identically(ops, train, monkeypatch):
    from macr_amd.mf import BPRMF
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")
    cfg = dict(n_users=40, n_items=50)
    a, b = BPRMF(_mf_args(), cfg, seed=7), BPRMF(_mf_args(), cfg, seed=7)
    monkeypatch.delenv("MACR_DETERMINISTIC")
    off = BPRMF(_mf_args(), cfg, seed=7)
    assert a.deterministic and b.deterministic and not off.deterministic
    assert BPRMF(_mf_args(), cfg, seed=7, deterministic=True).deterministic               # the keyword, without the variable
    kind = a.kind_of(train)
    for u, i, j in problem("B300")[4][:5]:                       # hot-row batches: 40 users, 50 items
        for m in (a, b):
            m.train_step(kind, m.to_device_batch(u.tolist(), i.tolist(), j.tolist()), defer=True)
    assert all(st.deterministic and st.lazy_period == 1 for m in (a, b) for st in m._opt.values())
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa) == sorted(sb) and "opt%d.adam_pow" % kind in sa
    for k in sa:
        if torch.is_tensor(sa[k]):
            assert bits_equal(sa[k], sb[k]), k
        else:
            assert sa[k] == sb[k], k
    assert not torch.equal(sa["user_embedding"], off.user_embedding)          # (it trained)


def _cli_run(tmp):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp / "data" / "tiny_data")
    env = dict(os.environ, PYTHONUNBUFFERED="1", MACR_DETERMINISTIC="1")
    cmd = [sys.executable, os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp / "data") + "/", "--dataset", "tiny_data",
           "--batch_size", "16", "--cuda", "0", "--saveID", "det", "--log_interval", "1", "--lr", "0.01", "--epoch", "5",
           "--train", "rubibceboth", "--test", "rubi", "--c", "40", "--Ks", "[5]", "--save_flag", "1"]
    out = subprocess.run(cmd, cwd=str(tmp), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ckpts = {}
    for root, _, files in os.walk(str(tmp)):
        for f in files:
            if f.endswith("_ckpt.pt"):
                ckpts[f] = torch.load(os.path.join(root, f), map_location="cpu")
    return out.stdout, ckpts


def test_mf_cli_runs_are_bit_identical(tmp_path, record_property):
    from macr_amd.mf import deterministic_from_env          # noqa: F401  (the variable is the model's: nothing in the CLI reads it)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    (out_a, ck_a), (out_b, ck_b) = _cli_run(tmp_path / "a"), _cli_run(tmp_path / "b")
    assert sorted(ck_a) == sorted(ck_b) == ["%d_ckpt.pt" % e for e in range(5)], (sorted(ck_a), sorted(ck_b))
    for f in ck_a:
        assert sorted(ck_a[f]) == sorted(ck_b[f])
        for k, v in ck_a[f].items():
            if torch.is_tensor(v):
                assert bits_equal(v, ck_b[f][k]), (f, k)
            else:
                assert v == ck_b[f][k], (f, k)
    assert not torch.equal(ck_a["0_ckpt.pt"]["user_embedding"], ck_a["4_ckpt.pt"]["user_embedding"])
    train = lambda out: [l.split("train==[")[1].split("]")[0] for l in out.splitlines() if "train==[" in l]
    ta, tb = train(out_a), train(out_b)
    assert len(ta) == 5 and ta == tb, (ta, tb)
    whole = out_a.splitlines() == out_b.splitlines()         # (the lines carry wall-clock times: on record, not asserted)
    record_property("whole_lines_identical", whole)
    strip = lambda out: [l.split("]: ", 1)[-1] for l in out.splitlines() if "train==[" in l]
    record_property("lines_identical_without_times", strip(out_a) == strip(out_b))
    print("CLI: whole lines identical: %s; without the times: %s" % (whole, strip(out_a) == strip(out_b)))
