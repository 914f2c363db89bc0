"""Per-item accuracy diagnostic (--out 1) on the GPU: macr_item_counts against the NumPy restatement (tests/item_acc_ref.py),
Evaluator.item_accuracy against the restatement fed with ops.score_matrix's fp32 scores, and both CLIs.  Every comparison
is exact integer equality."""
import ast
import ctypes
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import item_acc_ref as R
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a5a5a5a


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def zipf_cdf(n_items):
    p = 1.0 / np.arange(1, n_items + 1)
    return np.cumsum(p / p.sum())


def synthetic(rs, U, K, n_items):
    """(rankings (U,K) int32, ground-truth lists): Zipf-drawn ids permuted over the catalogue, distinct within a list, -1
    tails of every length (whole lists of -1 among them), users without ground truth, ground truth that holds some of the
    user's ranked ids and some others"""
    cdf, relabel = zipf_cdf(n_items), rs.permutation(n_items)
    rankings = np.full((U, K), -1, dtype=np.int32)
    gt = []
    for q in range(U):
        draw = relabel[np.minimum(np.searchsorted(cdf, rs.random_sample(3 * K)), n_items - 1)]
        _, first = np.unique(draw, return_index=True)
        ids = draw[np.sort(first)]
        mode = rs.randint(0, 4)                   # 0: all -1, 1: a tail of -1, else as full as the draws allow
        L = 0 if mode == 0 else (rs.randint(0, K + 1) if mode == 1 else K)
        ids = ids[:min(L, len(ids))]
        rankings[q, :len(ids)] = ids
        if rs.randint(0, 5) == 0:
            gt.append([])
            continue
        mine = ids[rs.random_sample(len(ids)) < 0.3]
        other = relabel[np.minimum(np.searchsorted(cdf, rs.random_sample(rs.randint(0, 4))), n_items - 1)]
        gt.append(sorted(set(mine.tolist()) | set(other.tolist())))
    return rankings, gt


def raw_counts(ops, rankings, gt_csr, k, n_items, group_of=None, n_groups=0):
    """macr_item_counts through the C ABI on outputs pre-filled with garbage"""
    from macr_amd import _lib
    U, K = rankings.shape
    rec = torch.full((n_items,), GARBAGE, dtype=torch.int32, device="cuda")
    hit = torch.full((n_items,), GARBAGE, dtype=torch.int32, device="cuda")
    sums = torch.full((max(n_groups, 1), 2), GARBAGE, dtype=torch.int64, device="cuda") if group_of is not None else None
    L = _lib.lib()
    need = L.macr_item_counts_workspace_bytes(U, K, n_items)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(L.macr_item_counts(U, K, k, p(rankings), p(gt_csr.ptr), p(gt_csr.idx), n_items, p(group_of), n_groups,
                                  p(rec), p(hit), p(sums), p(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return rec.cpu().numpy(), hit.cpu().numpy(), None if sums is None else sums.cpu().numpy()


@pytest.mark.parametrize("n_items", [7, 744, 70001])
def test_item_counts_equals_the_restatement(ops, n_items):
    rs = np.random.RandomState(n_items)
    group_np = rs.randint(0, 6, n_items).astype(np.int32)
    group_of = dev(group_np)
    for U in (1, 63, 64, 65, 1000):
        for K, k in ((5, 5), (20, 1), (20, 20), (32, 20), (128, 5)):
            rankings, gt = synthetic(rs, U, K, n_items)
            want_rec, want_hit = R.item_counts(rankings, gt, k, n_items)
            want_sums = R.group_sums(group_np, want_rec, want_hit, 6)
            rk, gt_csr = dev(rankings), ops.CSR.from_lists(gt, "cuda")
            rec, hit, sums = raw_counts(ops, rk, gt_csr, k, n_items)
            assert sums is None
            assert np.array_equal(rec, want_rec) and np.array_equal(hit, want_hit), (U, K, k)
            rec2, hit2, sums2 = raw_counts(ops, rk, gt_csr, k, n_items, group_of, 6)
            assert np.array_equal(rec2, want_rec) and np.array_equal(hit2, want_hit), (U, K, k)
            assert np.array_equal(sums2, want_sums), (U, K, k)
            # the torch face, and the same call again: bit-identical
            for _ in range(2):
                a, b, c = ops.item_counts(rk, gt_csr, k, n_items, group_of, 6)
                assert np.array_equal(a.cpu().numpy(), want_rec) and np.array_equal(b.cpu().numpy(), want_hit)
                assert c.dtype == torch.int64 and np.array_equal(c.cpu().numpy(), want_sums)


def test_item_counts_under_contention(ops):
    """70 000 users share their first slot and hold it in their ground truth (a count above 65 535: no 16-bit bin survives
    it), 64 more items are in every user's list, and every list goes on with 63 ids of its own: 9 M entries, about 1 100
    distinct ids per workgroup against 2 048 bins of 4 probes, so part of the tail takes the kernel's direct global adds"""
    U, K, n_items = 70000, 128, 70001
    k = K
    rs = np.random.RandomState(5)
    hot = rs.permutation(n_items)[:65].astype(np.int32)           # hot[0]: everybody's first slot
    rankings = np.empty((U, K), dtype=np.int32)
    rankings[:, :65] = hot[None, :]
    tail = np.setdiff1d(np.arange(n_items, dtype=np.int32), hot)
    rankings[:, 65:] = tail[(np.arange(U)[:, None] * 63 + np.arange(63)[None, :]) % len(tail)]      # distinct within a row
    gt = [sorted([int(hot[0])] + ([int(hot[7])] if q % 3 == 0 else []) + ([int(rankings[q, 65 + q % 63])] if q % 5 == 0 else []))
          for q in range(U)]
    want_rec = np.bincount(rankings.ravel(), minlength=n_items).astype(np.int64)
    want_hit = np.bincount(rankings[np.arange(0, U, 5), 65 + np.arange(0, U, 5) % 63], minlength=n_items).astype(np.int64)
    want_hit[hot[0]] = U
    want_hit[hot[7]] = (U + 2) // 3
    group_np = (np.arange(n_items) % 6).astype(np.int32)
    rk, gt_csr = dev(rankings), ops.CSR.from_lists(gt, "cuda")
    for _ in range(2):
        rec, hit, sums = raw_counts(ops, rk, gt_csr, k, n_items, dev(group_np), 6)
        assert rec[hot[0]] == U and hit[hot[0]] == U and np.all(rec[hot] == U)
        assert np.array_equal(rec, want_rec) and np.array_equal(hit, want_hit)
        assert np.array_equal(sums, R.group_sums(group_np, want_rec, want_hit, 6))
    assert sums[:, 0].sum() == U * k
    # the restatement's own loop agrees with the closed form on a slice of the users
    sub_rec, sub_hit = R.item_counts(rankings[:500], gt[:500], k, n_items)
    rec, hit, _ = raw_counts(ops, dev(rankings[:500]), ops.CSR.from_lists(gt[:500], "cuda"), k, n_items)
    assert np.array_equal(rec, sub_rec) and np.array_equal(hit, sub_hit)


def random_mask(rs, U, n_items, mean_len, heavy=()):
    lists = []
    for q in range(U):
        n = n_items - 4 if q in heavy else min(int(rs.poisson(mean_len)), n_items)       # heavy: 4 candidates left (< K)
        lists.append(sorted(rs.choice(n_items, size=n, replace=False).tolist()))
    return lists


@pytest.mark.parametrize("filt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
@pytest.mark.parametrize("U,N,d", [(300, 744, 64), (70, 25, 32)])
def test_evaluator_item_accuracy(ops, monkeypatch, U, N, d, kind_name, filt):
    from macr_amd.evaluator import Evaluator
    monkeypatch.setenv("MACR_EVAL_FILTER", filt)
    kind = getattr(ops, kind_name)
    rs = np.random.RandomState(U + N + d)
    n_users = U + 20
    P = dev((rs.standard_normal((n_users, d)) * 0.5).astype(np.float32))
    Qn = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    Qn += (rs.standard_normal(N).astype(np.float32) * 0.5)[:, None] * np.sign(P.cpu().numpy().mean(0, keepdims=True))    # popularity
    Q = dev(Qn)
    w = dev((rs.standard_normal(d) * 0.3).astype(np.float32))
    wu = dev((rs.standard_normal(d) * 0.3).astype(np.float32))
    uid_np = rs.permutation(n_users)[:U].astype(np.int32)
    uid = dev(uid_np)
    mask = random_mask(rs, U, N, 6 if N < 100 else 12, heavy=(0, U - 1))
    gt = [sorted(set(rs.randint(0, N, rs.randint(1, 6)).tolist())) for _ in range(U)]
    c = 0.7
    sig_i = sig_u = None
    if kind != ops.SCORE_NORMAL:
        sig_i, sig_u = ops.branch_sigmoid(Q, w), ops.branch_sigmoid(P, wu, uid)
    scores = ops.score_matrix(kind, P, uid, Q, sig_u, sig_i, c).cpu().numpy()
    group_np = rs.randint(0, 6, N).astype(np.int32)
    ev = Evaluator(mask, gt, N, "cuda")
    assert ev.filter == filt
    for k in (5, 20, 5):                           # N = 25: fewer than 20 candidates for several users, 4 for two of them;
        # the second k = 5 counts the head of a ranking of depth 20 (the evaluator's last depth)
        want_rec, want_hit = R.item_counts(R.rank_outside_train(scores, mask, k), gt, k, N)
        rec, hit, sums = ev.item_accuracy(kind, P, uid, Q, k, w, wu, c, group_of=group_np, n_groups=6)
        assert np.array_equal(rec.cpu().numpy(), want_rec) and np.array_equal(hit.cpu().numpy(), want_hit), k
        assert np.array_equal(sums.cpu().numpy(), R.group_sums(group_np, want_rec, want_hit, 6))
    assert want_rec.sum() == sum(min(5, N - len(m)) for m in mask)
    rec, hit, none = ev.item_accuracy(kind, P, uid, Q, 20, w, wu, c)
    want_rec, want_hit = R.item_counts(R.rank_outside_train(scores, mask, 20), gt, 20, N)
    assert none is None and np.array_equal(rec.cpu().numpy(), want_rec) and np.array_equal(hit.cpu().numpy(), want_hit)
    # the item table cut into two simulated shards: each ranks its rows, the merged ranking counts the same
    parts = []
    for lo, hi in ((0, N // 3), (N // 3, N)):
        e = Evaluator(mask, gt, N, "cuda")
        e.local_items_range = (lo, hi)
        parts.append(e.rank_local(kind, P, uid, Q[lo:hi].contiguous(), 20, w, wu, c))
    _, mi, _ = ops.topk_merge(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    srec, shit, _ = ops.item_counts(mi, ev.gt, 20, N)
    assert torch.equal(srec, rec) and torch.equal(shit, hit)


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _metric_lines(out, marker):
    """the evaluation lines without their wall-clock brackets"""
    lines = [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if marker in l and "recall=[" in l]
    assert len(lines) == 2, out
    return lines


def test_mf_cli_out_flag(ops, tmp_path):
    from macr_amd.data import MFData
    from macr_amd.mf import BPRMF
    on, off = tmp_path / "on", tmp_path / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    flags = lambda d, o: ["--data_path", str(d / "data") + "/", "--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0",
                          "--saveID", "d", "--log_interval", "2", "--lr", "0.01", "--epoch", "4", "--train", "normalbce",
                          "--test", "normal", "--Ks", "[5, 20]", "--save_flag", "1", "--verbose", "1", "--out", str(o)]
    out1 = _run([os.path.join(REPO, "macr_mf", "train.py")] + flags(on, 1), str(on))
    out0 = _run([os.path.join(REPO, "macr_mf", "train.py")] + flags(off, 0), str(off))
    assert _metric_lines(out1, "train==[") == _metric_lines(out0, "train==[")
    assert out1.count("item groups @5: catalogue=[") == 2 and "item groups" not in out0
    assert not os.path.exists(off / "MF_macr.txt") and not glob.glob(str(off / "*macr.txt"))
    got = ast.literal_eval(open(on / "MF_macr.txt").read())
    # the restatement on the saved model's ratings
    args = _load(os.path.join(REPO, "macr_mf", "parse.py"), "mf_parse_for_item_acc").parse_args(flags(on, 1))
    data = MFData(args)
    model = BPRMF(args, dict(n_users=data.n_users, n_items=data.n_items))
    ckpt = glob.glob(str(on / "*_checkpoint" / "*" / "3_ckpt.pt"))
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    users = list(data.test_user_list.keys())
    scores = model.ratings(ops.SCORE_NORMAL, users).cpu().numpy()
    train, test = data.eval_lists(users)
    rec, hit, n_test, want = R.item_accuracy(scores, train, test, 5)
    assert got == want and str(got) == str(want) and len(got) == data.n_items
    groups = R.groups_of([len(data.train_item_list.get(i, ())) for i in range(data.n_items)])
    rows = R.group_table(groups, rec, hit, n_test)
    line = [l for l in out1.splitlines() if l.startswith("item groups @5")][-1]
    assert line.endswith("recall=[%s]" % ", ".join("%.5f" % r["recall"] for r in rows)), line
    assert "slots=[%s]" % ", ".join("%.5f" % r["slot_share"] for r in rows) in line, line


def test_lightgcn_cli_out_flag(ops, tmp_path):
    from macr_amd.data import LGCNData
    from macr_amd.lightgcn import LightGCN
    on, off = tmp_path / "on", tmp_path / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    flags = lambda d, o: ["--data_path", str(d / "data") + "/", "--dataset", "tiny_data", "--verbose", "1", "--layer_size", "[64,64]",
                          "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0", "--epoch", "4", "--log_interval", "2",
                          "--weights_path", str(d) + "/", "--saveID", "d", "--loss", "bce", "--test", "normal", "--out", str(o)]
    out1 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(on, 1), str(on))
    out0 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(off, 0), str(off))
    assert _metric_lines(out1, "test==[") == _metric_lines(out0, "test==[")
    assert out1.count("item groups @20: catalogue=[") == 2 and "item groups" not in out0
    assert not glob.glob(str(off / "*macr.txt"))
    got = ast.literal_eval(open(on / "Lightgcn_macr.txt").read())
    args = _load(os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"), "lgcn_parser_for_item_acc").parse_args(flags(on, 1))
    assert args.adj_type == "pre"
    data = LGCNData(args.data_path + args.dataset, args.batch_size, args)
    model = LightGCN(dict(n_users=data.n_users, n_items=data.n_items, norm_adj=data.get_adj_mat()[3]), args)
    ckpt = glob.glob(str(on / "weights" / "**" / "weights_d-4.pt"), recursive=True)
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    users = list(data.test_set.keys())
    scores = model.ratings(ops.SCORE_NORMAL, users).cpu().numpy()
    train, test = data.eval_lists(users)
    rec, hit, n_test, want = R.item_accuracy(scores, train, test, 20)
    assert got == want and str(got) == str(want) and len(got) == data.n_items
