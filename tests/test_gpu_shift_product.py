"""The list shift report (MACR_SHIFT_REPORT) through the product: the line of both command lines against a recomputation from
the saved checkpoint (oracle.score_matrix, a full sort under the project's tie rule, tests/shift_ref.py, then
macr_amd/shift_report.py), the runs' other lines against a run without the variable, the notice under --test normal, the depth
part and its refusal on row shards, and the same line from one process, from a row-sharded model and from two ranks.
Training runs under MACR_DETERMINISTIC=1, so that a run with the variable and a run without it are comparable."""
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

import item_acc_ref
import oracle
import shift_ref as R
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu

K = 10          # max(--Ks): below most users' candidate counts on the tiny dataset (25 items), so that lists can differ as sets


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def _env(report, training=True, **extra):
    """training: the run trains, under MACR_DETERMINISTIC=1 (a --pretrain 1 run only evaluates, and the row-sharded model refuses
    that variable)"""
    env = dict(os.environ, PYTHONUNBUFFERED="1", **extra)
    env.pop("MACR_SHIFT_REPORT", None)
    env.pop("MACR_DETERMINISTIC", None)
    if training:
        env["MACR_DETERMINISTIC"] = "1"
    if report:
        env["MACR_SHIFT_REPORT"] = str(report)
    return env


def _run(cmd, cwd, report, ok=True, training=True):
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=_env(report, training), capture_output=True, text=True, timeout=300)
    assert (out.returncode == 0) == ok, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout if ok else out.stderr


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lines(out):
    return [l for l in out.splitlines() if l.startswith("shift @")]


def _other_lines(out):
    return [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if not l.startswith("shift @")]


def _recomputed_line(base_scores, here_scores, train, test, n_items, train_counts, k):
    """the shift line from two score matrices of the oracle: full sorts outside the train lists (score descending, ties by
    ascending id), the restatement's comparison, plain-loop counts, the report"""
    from macr_amd import shift_report
    base = item_acc_ref.rank_outside_train(base_scores, train, k)
    here = item_acc_ref.rank_outside_train(here_scores, train, k)
    per_user, entered, left = R.list_shift(base, here, test, k, n_items)
    e_rec, e_hit = item_acc_ref.item_counts(entered, test, k, n_items)
    l_rec, l_hit = item_acc_ref.item_counts(left, test, k, n_items)
    group_of = item_acc_ref.groups_of(train_counts)
    return shift_report.format_line(shift_report.summarize(per_user, e_rec, e_hit, l_rec, l_hit, group_of, 6, k)), per_user, entered


LINE = (r"shift @10 vs normal: users=\d+ identical=\d+ overlap=\d\.\d{5} first_diff=\d+\.\d{3} footrule=[0-9.na]+ \| "
        r"hits base=\d+ here=\d+ kept=\d+ gained=\d+ lost=\d+ users better=\d+ worse=\d+ sign_p=[0-9.e-]+ \| "
        r"train-popularity groups \(<10,<50,<100,<200,<500,>=500\): entered=\[[0-9.na, ]+\] left=\[[0-9.na, ]+\] "
        r"gained=\[\d+(, \d+){5}\] lost=\[\d+(, \d+){5}\]")
DEPTH = r" \| depth: entered med=(\d+|nan) p90=(\d+|nan) max=(\d+|nan) left med=(\d+|nan) p90=(\d+|nan) max=(\d+|nan) \(skipped=\d+\)"

MF_FLAGS = ["--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0", "--saveID", "d", "--log_interval", "1", "--lr", "0.01",
            "--epoch", "3", "--train", "rubibceboth", "--test", "rubi", "--c", "0.5", "--Ks", "[5, 10]", "--save_flag", "1",
            "--verbose", "1"]


def _mf_cmd(d):
    return [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(d / "data") + "/"] + MF_FLAGS


@pytest.fixture(scope="module")
def mf_runs(ops, tmp_path_factory):
    """the MF command line for 3 epochs with and without the variable -> (directory of the run with it, its stdout, the other's)"""
    root = tmp_path_factory.mktemp("shift_mf")
    on, off = root / "on", root / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    return on, _run(_mf_cmd(on), str(on), 1), _run(_mf_cmd(off), str(off), 0)


def test_mf_cli_shift_report(ops, mf_runs):
    from macr_amd.data import MFData
    from macr_amd.mf import BPRMF
    on, out1, out0 = mf_runs
    lines = _lines(out1)
    assert len(lines) == 3 and "shift @" not in out0 and "MACR_SHIFT_REPORT" not in out0, out1     # one per evaluation; unset: none
    assert _other_lines(out1) == _other_lines(out0) and sum("recall=[" in l for l in out0.splitlines()) == 3
    args = _load(os.path.join(REPO, "macr_mf", "parse.py"), "mf_parse_for_shift").parse_args(
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
    here = oracle.score_matrix(oracle.SCORE_RUBI_BOTH, Pn[users], Qn, sig_u, sig_i, 0.5)
    base = oracle.score_matrix(oracle.SCORE_NORMAL, Pn[users], Qn)
    train, test = data.eval_lists(users)
    counts = [len(data.train_item_list.get(i, ())) for i in range(data.n_items)]
    want, per_user, entered = _recomputed_line(base, here, train, test, data.n_items, counts, K)
    assert lines[-1] == want
    assert re.fullmatch(LINE, lines[-1]), lines[-1]
    assert "users=%d " % len(users) in lines[-1]
    assert (per_user[:, 3] < K).any()                                       # the corrected lists do differ from the factual ones


def test_mf_cli_normal_test_prints_the_notice_and_no_line(ops, tmp_path):
    from macr_amd import shift_report
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    cmd = [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset", "tiny_data",
           "--batch_size", "16", "--cuda", "0", "--log_interval", "1", "--epoch", "2", "--train", "normalbce", "--test", "normal",
           "--Ks", "[5, 10]", "--verbose", "1"]
    out = _run(cmd, str(tmp_path), 1)
    assert out.count(shift_report.NOTHING_TO_COMPARE) == 1 and not _lines(out), out
    assert sum("recall=[" in l for l in out.splitlines()) == 2


@pytest.fixture(scope="module")
def pretrain_line(ops, mf_runs):
    """--pretrain 1 on the run's checkpoint with value 1, one process -> (the command, its shift lines)"""
    on, out1, _ = mf_runs
    cmd = _mf_cmd(on) + ["--pretrain", "1"]
    one = _lines(_run(cmd, str(on), 1, training=False))
    assert len(one) == 1 and one[0] == _lines(out1)[-1]                     # (the newest checkpoint is the last evaluation's model)
    return cmd, one


def test_mf_cli_depth_part_and_its_refusal_on_row_shards(ops, mf_runs, pretrain_line):
    """MACR_SHIFT_REPORT=2: the value-1 line with the depth part behind it, and under --row_shard 1 a refusal that points to value 1"""
    on, (cmd, one) = mf_runs[0], pretrain_line
    deep = _lines(_run(cmd, str(on), 2, training=False))
    assert len(deep) == 1 and deep[0].startswith(one[0] + " | depth: ") and re.fullmatch(LINE + DEPTH, deep[0]), deep
    figures = re.fullmatch(LINE + DEPTH, deep[0]).groups()[-6:]
    for med, p90, top in (figures[:3], figures[3:]):
        assert (med, p90, top) == ("nan",) * 3 or int(med) <= int(p90) <= int(top)
    err = _run(cmd + ["--row_shard", "1"], str(on), 2, ok=False, training=False)
    assert "MACR_SHIFT_REPORT=2" in err and "--row_shard 1" in err and "MACR_SHIFT_REPORT=1" in err, err[-2000:]


def test_mf_cli_same_line_from_row_shards_and_from_two_ranks(ops, mf_runs, pretrain_line):
    """Value 1 from one process, from one process with --row_shard 1 and from two ranks (gloo rig, both on this GPU): the same
    line, character for character -- integers over the merged rankings"""
    on, (cmd, one) = mf_runs[0], pretrain_line
    sharded = _lines(_run(cmd + ["--row_shard", "1"], str(on), 1, training=False))
    assert sharded == one
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29563"] + cmd, cwd=str(on),
                         env=_env(1, training=False, MACR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    assert _lines(two.stdout) == one, two.stdout                            # the main rank alone prints, and prints the same


def test_lightgcn_cli_shift_report(ops, tmp_path):
    from macr_amd.data import LGCNData
    from macr_amd.lightgcn import LightGCN
    on = tmp_path / "on"
    shutil.copytree(os.path.join(GOLD, "tiny_data"), on / "data" / "tiny_data")
    flags = ["--data_path", str(on / "data") + "/", "--dataset", "tiny_data", "--verbose", "1", "--layer_size", "[64,64]",
             "--Ks", "[5, 10]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0", "--epoch", "3", "--log_interval", "1",
             "--weights_path", str(on) + "/", "--saveID", "d", "--loss", "bceboth", "--test", "rubiboth", "--c", "0.5"]
    out1 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags, str(on), 1)
    lines = _lines(out1)
    assert len(lines) == 3, out1                                            # one per evaluation
    args = _load(os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"), "lgcn_parser_for_shift").parse_args(flags)
    data = LGCNData(args.data_path + args.dataset, args.batch_size, args)
    model = LightGCN(dict(n_users=data.n_users, n_items=data.n_items, norm_adj=data.get_adj_mat()[3]), args)
    ckpt = glob.glob(str(on / "weights" / "**" / "weights_d-3.pt"), recursive=True)
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    users = list(data.test_set.keys())
    ua, ia = model.propagated()
    Pn, Qn = ua.cpu().numpy(), ia.cpu().numpy()
    sig_i = oracle.branch_sigmoid(Qn, model.w.cpu().numpy())
    sig_u = oracle.branch_sigmoid(Pn[users], model.w_user.cpu().numpy())
    here = oracle.score_matrix(oracle.SCORE_RUBI_BOTH, Pn[users], Qn, sig_u, sig_i, 0.5)
    base = oracle.score_matrix(oracle.SCORE_NORMAL, Pn[users], Qn)
    train, test = data.eval_lists(users)
    counts = np.zeros(data.n_items, dtype=np.int64)
    for items in data.train_items.values():
        np.add.at(counts, np.asarray(items, dtype=np.int64), 1)
    want, _, _ = _recomputed_line(base, here, train, test, data.n_items, counts, K)
    assert lines[-1] == want
    assert re.fullmatch(LINE, lines[-1]), lines[-1]
