"""The exposure report (MACR_EXPOSURE_REPORT=1) through the product: Evaluator.item_exposure against the restatement
(tests/exposure_ref.py) applied to Evaluator.rank's ids, the line of both command lines against a recomputation from the saved
checkpoint (oracle.score_matrix, a full sort under the project's tie rule, the restatement), and the same line from two
ranks and from a row-sharded model."""
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import exposure_ref as R
import item_acc_ref
import oracle
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- the evaluator
@pytest.fixture(scope="module")
def mf_model(ops):
    """300 query users of 320 x 2000 items, d = 64, item rows with a popularity direction"""
    from macr_amd.mf import BPRMF
    rs = np.random.RandomState(21)
    n_users, N, d = 320, 2000, 64
    P = (rs.standard_normal((n_users, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    Q += (rs.standard_normal(N).astype(np.float32) * 0.5)[:, None] * np.sign(P.mean(0, keepdims=True))
    w, wu = ((rs.standard_normal(d) * 0.3).astype(np.float32) for _ in range(2))
    args = types.SimpleNamespace(regs=1e-5, embed_size=d, lr=1e-3, batch_size=32, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)
    model = BPRMF(args, dict(n_users=n_users, n_items=N),
                  weights={"user_embedding": P, "item_embedding": Q, "w": w.reshape(-1, 1), "w_user": wu.reshape(-1, 1)})
    model.update_c(None, 0.7)
    uid_np = rs.permutation(n_users)[:300].astype(np.int32)
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(300)]
    gt = [sorted(set(rs.randint(0, N, rs.randint(0, 6)).tolist())) for _ in range(300)]
    return model, uid_np, mask, gt, N


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_evaluator_item_exposure(ops, mf_model, kind_name):
    from macr_amd import exposure
    from macr_amd.evaluator import Evaluator
    model, uid_np, mask, gt, N = mf_model
    kind, uid = getattr(ops, kind_name), dev(uid_np)
    group_np = (np.arange(N) * 7 % 6).astype(np.int32)
    args = (kind, model.user_embedding, uid, model.item_embedding)
    # every seventh user also holds one of its own ranked ids, so that hits exist at every list position whatever the model
    _, idx, _ = Evaluator(mask, gt, N, "cuda").rank(*args, 20, w=model.w, wu=model.w_user, c=model.rubi_c)
    first = idx.cpu().numpy()
    gt = [sorted(set(row) | {int(first[u, u % 20])}) if u % 7 == 0 else row for u, row in enumerate(gt)]
    ev = Evaluator(mask, gt, N, "cuda")
    for k in (20, 5):                               # the second: the head of a ranking of depth 20 (the evaluator's last depth)
        _, idx, _ = ev.rank(*args, 20, w=model.w, wu=model.w_user, c=model.rubi_c)
        ids = idx.cpu().numpy()
        assert np.array_equal(ids, first)
        want_e, want_h = R.item_exposure(ids, gt, R.weights(k), N)
        assert want_h.any()
        want_rec, _ = item_acc_ref.item_counts(ids, gt, k, N)
        rec, exp_w, hit_w, sums = ev.item_exposure(*args, k, model.w, model.w_user, model.rubi_c, group_of=group_np, n_groups=6)
        assert rec.dtype == torch.int32 and exp_w.dtype == hit_w.dtype == sums.dtype == torch.int64
        assert np.array_equal(rec.cpu().numpy(), want_rec)
        assert np.array_equal(exp_w.cpu().numpy(), want_e) and np.array_equal(hit_w.cpu().numpy(), want_h)
        assert np.array_equal(sums.cpu().numpy(), R.group_sums(group_np, want_e, want_h, 6))
        assert want_e.sum() == 300 * int(R.weights(k).astype(np.int64).sum())             # every slot filled and weighted
        train = np.arange(N) % 700
        got = exposure.summarize(rec.cpu().numpy(), exp_w.cpu().numpy(), hit_w.cpu().numpy(), train, group_np, 6, 300, k)
        assert exposure.format_line(got) == R.format_line(R.summarize(want_rec, want_e, want_h, train, group_np, 6, 300, k))
        # the group shares are the device's group sums
        assert np.array_equal(got["group_exposure"], sums.cpu().numpy()[:, 0] / float(want_e.sum()))
    _, _, _, none = ev.item_exposure(*args, 20, model.w, model.w_user, model.rubi_c)
    assert none is None
    # the item table cut into two simulated shards: each ranks its rows, the merged ranking weighs the same
    parts = []
    for lo, hi in ((0, N // 3), (N // 3, N)):
        e = Evaluator(mask, gt, N, "cuda")
        e.local_items_range = (lo, hi)
        parts.append(e.rank_local(kind, model.user_embedding, uid, model.item_embedding[lo:hi].contiguous(), 20, model.w,
                                  model.w_user, model.rubi_c))
    _, mi, _ = ops.topk_merge(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]))
    se, sh, _ = ops.item_exposure(mi, ev.gt, R.weights(20), N)
    want_e, want_h = R.item_exposure(ids, gt, R.weights(20), N)
    assert np.array_equal(se.cpu().numpy(), want_e) and np.array_equal(sh.cpu().numpy(), want_h)


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _env(report, **extra):
    env = dict(os.environ, PYTHONUNBUFFERED="1", **extra)
    env.pop("MACR_EXPOSURE_REPORT", None)
    if report:
        env["MACR_EXPOSURE_REPORT"] = "1"
    return env


def _run(cmd, cwd, report):
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=_env(report), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lines(out):
    return [l for l in out.splitlines() if l.startswith("exposure @")]


def _metric_lines(out):
    return [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if "recall=[" in l]


def _recomputed_line(scores, train, test, n_items, train_counts, k):
    """the exposure line from a score matrix of the oracle: full sort outside the train lists (score descending, ties by
    ascending id), the restatement's sums and report"""
    ids = item_acc_ref.rank_outside_train(scores, train, k)
    exp_w, hit_w = R.item_exposure(ids, test, R.weights(k), n_items)
    rec, _ = item_acc_ref.item_counts(ids, test, k, n_items)
    group_of = item_acc_ref.groups_of(train_counts)
    return R.format_line(R.summarize(rec, exp_w, hit_w, train_counts, group_of, 6, len(train), k))


LINE = (r"exposure @20: users=\d+ slots=\d+ coverage=\d\.\d{5} gini=\d\.\d{5} gini_dcg=\d\.\d{5} arp=\d+\.\d\d arp_dcg=\d+\.\d\d \| "
        r"train-popularity groups \(<10,<50,<100,<200,<500,>=500\): exposure=\[[0-9.na, ]+\] dcg_hits=\[[0-9.na, ]+\]")

MF_FLAGS = ["--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0", "--saveID", "d", "--log_interval", "1", "--lr", "0.01",
            "--epoch", "3", "--train", "rubibceboth", "--test", "rubi", "--c", "0.5", "--Ks", "[5, 20]", "--save_flag", "1",
            "--verbose", "1"]


@pytest.fixture(scope="module")
def mf_runs(ops, tmp_path_factory):
    """the MF command line for 3 epochs with and without the variable -> (directory of the run with it, its stdout, the other's)"""
    root = tmp_path_factory.mktemp("exposure_mf")
    on, off = root / "on", root / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    cmd = lambda d: [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(d / "data") + "/"] + MF_FLAGS
    return on, _run(cmd(on), str(on), True), _run(cmd(off), str(off), False)


def test_mf_cli_exposure_report(ops, mf_runs):
    from macr_amd.data import MFData
    from macr_amd.mf import BPRMF
    on, out1, out0 = mf_runs
    lines = _lines(out1)
    assert len(lines) == 3 and "exposure @" not in out0, out1               # one per evaluation; none without the variable
    assert _metric_lines(out1) == _metric_lines(out0) and len(_metric_lines(out0)) == 3      # the evaluation itself is untouched
    args = _load(os.path.join(REPO, "macr_mf", "parse.py"), "mf_parse_for_exposure").parse_args(
        ["--data_path", str(on / "data") + "/"] + MF_FLAGS)
    data = MFData(args)
    model = BPRMF(args, dict(n_users=data.n_users, n_items=data.n_items))
    ckpt = glob.glob(str(on / "*_checkpoint" / "*" / "2_ckpt.pt"))
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    assert model.rubi_c == 0.5
    users = list(data.test_user_list.keys())
    Pn, Qn = model.user_embedding.cpu().numpy(), model.item_embedding.cpu().numpy()
    sig_i = oracle.branch_sigmoid(Qn, model.w.cpu().numpy())
    sig_u = oracle.branch_sigmoid(Pn[users], model.w_user.cpu().numpy())
    scores = oracle.score_matrix(oracle.SCORE_RUBI_BOTH, Pn[users], Qn, sig_u, sig_i, 0.5)
    train, test = data.eval_lists(users)
    counts = [len(data.train_item_list.get(i, ())) for i in range(data.n_items)]
    assert lines[-1] == _recomputed_line(scores, train, test, data.n_items, counts, 20)
    assert re.fullmatch(LINE, lines[-1]), lines[-1]
    assert "users=%d " % len(users) in lines[-1]


def test_mf_cli_same_line_from_two_ranks_and_from_row_shards(ops, mf_runs):
    """--pretrain 1 on the run's checkpoint: one process, one process with --row_shard 1, and two ranks (gloo rig, both on this
    GPU) rank the same model and print the same line -- the sums are integers over the merged ranking"""
    on, out1, _ = mf_runs
    cmd = [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(on / "data") + "/"] + MF_FLAGS + ["--pretrain", "1"]
    one = _lines(_run(cmd, str(on), True))
    assert len(one) == 1 and one[0] == _lines(out1)[-1]                     # (the newest checkpoint is the last evaluation's model)
    sharded = _lines(_run(cmd + ["--row_shard", "1"], str(on), True))
    assert sharded == one
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29561"] + cmd, cwd=str(on),
                         env=_env(True, MACR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=600)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    assert _lines(two.stdout) == one, two.stdout                            # the main rank alone prints, and prints the same


def test_lightgcn_cli_exposure_report(ops, tmp_path):
    from macr_amd.data import LGCNData
    from macr_amd.lightgcn import LightGCN
    on, off = tmp_path / "on", tmp_path / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    flags = lambda d: ["--data_path", str(d / "data") + "/", "--dataset", "tiny_data", "--verbose", "1", "--layer_size", "[64,64]",
                       "--Ks", "[5, 20]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0", "--epoch", "3", "--log_interval", "1",
                       "--weights_path", str(d) + "/", "--saveID", "d", "--loss", "bce", "--test", "normal"]
    out1 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(on), str(on), True)
    out0 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(off), str(off), False)
    lines = _lines(out1)
    assert len(lines) == 3 and "exposure @" not in out0, out1
    assert _metric_lines(out1) == _metric_lines(out0) and len(_metric_lines(out0)) == 3
    args = _load(os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"), "lgcn_parser_for_exposure").parse_args(flags(on))
    data = LGCNData(args.data_path + args.dataset, args.batch_size, args)
    model = LightGCN(dict(n_users=data.n_users, n_items=data.n_items, norm_adj=data.get_adj_mat()[3]), args)
    ckpt = glob.glob(str(on / "weights" / "**" / "weights_d-3.pt"), recursive=True)
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    users = list(data.test_set.keys())
    ua, ia = model.propagated()
    scores = oracle.score_matrix(oracle.SCORE_NORMAL, ua.cpu().numpy()[users], ia.cpu().numpy())
    train, test = data.eval_lists(users)
    counts = np.zeros(data.n_items, dtype=np.int64)
    for items in data.train_items.values():
        np.add.at(counts, np.asarray(items, dtype=np.int64), 1)
    assert lines[-1] == _recomputed_line(scores, train, test, data.n_items, counts, 20)
    assert re.fullmatch(LINE, lines[-1]), lines[-1]
