"""The calibration report (MACR_CALIBRATION_REPORT) through the product: the line of both command lines against a recomputation
from the saved checkpoint (oracle.score_matrix, a full sort under the project's tie rule, tests/calibration_ref.py), the runs'
other lines against a run without the variable, value 2 and its notice under --test normal, the tuners' one line per
evaluation, and the same line from one process, from a row-sharded model and from two ranks.
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

import calibration_ref as R
import item_acc_ref
import oracle
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu

K = 10          # max(--Ks): below most users' candidate counts on the tiny dataset (25 items)


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
    env.pop("MACR_CALIBRATION_REPORT", None)
    env.pop("MACR_DETERMINISTIC", None)
    if training:
        env["MACR_DETERMINISTIC"] = "1"
    if report:
        env["MACR_CALIBRATION_REPORT"] = str(report)
    return env


def _run(cmd, cwd, report, training=True):
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=_env(report, training), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lines(out):
    return [l for l in out.splitlines() if l.startswith("calibration @")]


def _other_lines(out):
    return [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if not l.startswith("calibration @")]


def _recomputed_line(here_scores, base_scores, train, test, n_items, train_counts, k):
    """the line from the oracle's score matrices: full sorts outside the train lists (score descending, ties by ascending id),
    the restatement's counts and report; base_scores None: value 1"""
    from macr_amd import calibration
    counts = np.asarray(train_counts, dtype=np.int64)
    group_of = item_acc_ref.groups_of(counts)
    p_cnt, _, p_wsum = R.group_hist(train, group_of, 6, n_items, item_weight=counts)
    sides = [None if s is None else R.group_hist(item_acc_ref.rank_outside_train(s, train, k), group_of, 6, n_items, test, counts, k=k)
             for s in (here_scores, base_scores)]
    rep = R.summarize((p_cnt, p_wsum), sides[0], [len(t) for t in test], k, sides[1])
    return calibration.format_line(rep), rep


NUM = r"(-?\d+\.\d+|nan)"
TRIPLE = r"\[%s, %s, %s\]" % (NUM, NUM, NUM)
LINE = (r"calibration @10: users=\d+ skipped=\d+ js=%s tv=%s gap_profile=%s gap_list=%s lift=%s \| users by profile popularity "
        r"\(niche 20%%, diverse 60%%, blockbuster 20%%\): users=\[\d+, \d+, \d+\] js=%s lift=%s recall=%s"
        % (NUM, NUM, NUM, NUM, NUM, TRIPLE, TRIPLE, TRIPLE))
BASE = r" \| normal: js=%s tv=%s gap_list=%s lift=%s js=%s lift=%s recall=%s" % (NUM, NUM, NUM, NUM, TRIPLE, TRIPLE, TRIPLE)

MF_FLAGS = ["--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0", "--saveID", "d", "--log_interval", "1", "--lr", "0.01",
            "--epoch", "3", "--train", "rubibceboth", "--test", "rubi", "--c", "0.5", "--Ks", "[5, 10]", "--save_flag", "1",
            "--verbose", "1"]


def _mf_cmd(d, script="train.py"):
    return [os.path.join(REPO, "macr_mf", script), "--data_path", str(d / "data") + "/"] + MF_FLAGS


@pytest.fixture(scope="module")
def mf_runs(ops, tmp_path_factory):
    """the MF command line for 3 epochs with and without the variable -> (directory of the run with it, its stdout, the other's)"""
    root = tmp_path_factory.mktemp("calibration_mf")
    on, off = root / "on", root / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    return on, _run(_mf_cmd(on), str(on), 1), _run(_mf_cmd(off), str(off), 0)


@pytest.fixture(scope="module")
def mf_checkpoint(ops, mf_runs):
    """the last checkpoint of the run, scored by the oracle -> (here scores, base scores, train, test, n_items, train counts)"""
    from macr_amd.data import MFData
    from macr_amd.mf import BPRMF
    on = mf_runs[0]
    args = _load(os.path.join(REPO, "macr_mf", "parse.py"), "mf_parse_for_calibration").parse_args(
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
    return here, base, train, test, data.n_items, counts


def test_mf_cli_calibration_report(ops, mf_runs, mf_checkpoint):
    on, out1, out0 = mf_runs
    lines = _lines(out1)
    assert len(lines) == 3 and "calibration @" not in out0 and "MACR_CALIBRATION_REPORT" not in out0, out1     # one per evaluation; unset: none
    assert _other_lines(out1) == _other_lines(out0) and sum("recall=[" in l for l in out0.splitlines()) == 3
    here, base, train, test, n_items, counts = mf_checkpoint
    want, rep = _recomputed_line(here, None, train, test, n_items, counts, K)
    assert lines[-1] == want
    assert re.fullmatch(LINE, lines[-1]), lines[-1]
    assert rep["skipped"] >= 1 and any(len(t) == 0 for t in train)          # the dataset's test user without a train list
    assert "users=%d skipped=%d " % (len(train) - rep["skipped"], rep["skipped"]) in lines[-1]


@pytest.fixture(scope="module")
def pretrain_line(ops, mf_runs):
    """--pretrain 1 on the run's checkpoint with value 1, one process -> (the command, its calibration lines)"""
    on, out1, _ = mf_runs
    cmd = _mf_cmd(on) + ["--pretrain", "1"]
    one = _lines(_run(cmd, str(on), 1, training=False))
    assert len(one) == 1 and one[0] == _lines(out1)[-1]                     # (the newest checkpoint is the last evaluation's model)
    return cmd, one


def test_mf_cli_value_2_adds_the_factual_rankings_figures(ops, mf_runs, mf_checkpoint, pretrain_line):
    on, (cmd, one) = mf_runs[0], pretrain_line
    out = _run(cmd, str(on), 2, training=False)
    both = _lines(out)
    here, base, train, test, n_items, counts = mf_checkpoint
    want, _ = _recomputed_line(here, base, train, test, n_items, counts, K)
    assert both == [want] and both[0].startswith(one[0] + " | normal: js=") and re.fullmatch(LINE + BASE, both[0]), both
    assert "MACR_CALIBRATION_REPORT" not in out                             # no notice: there is a ranking to compare with


def test_mf_cli_normal_test_with_value_2_prints_the_notice_and_the_value_1_line(ops, tmp_path):
    from macr_amd import calibration
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    cmd = [os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/", "--dataset", "tiny_data",
           "--batch_size", "16", "--cuda", "0", "--log_interval", "1", "--epoch", "2", "--train", "normalbce", "--test", "normal",
           "--Ks", "[5, 10]", "--verbose", "1"]
    out = _run(cmd, str(tmp_path), 2)
    lines = _lines(out)
    assert out.count(calibration.BASE_IS_THE_LIST) == 1 and len(lines) == 2, out
    assert all(re.fullmatch(LINE, l) for l in lines), lines


def test_mf_cli_same_line_from_row_shards_and_from_two_ranks(ops, mf_runs, pretrain_line):
    """Value 1 from one process, from one process with --row_shard 1 and from two ranks (gloo rig, both on this GPU): the same
    line, character for character -- integers over the merged rankings and the global-id train lists"""
    on, (cmd, one) = mf_runs[0], pretrain_line
    sharded = _lines(_run(cmd + ["--row_shard", "1"], str(on), 1, training=False))
    assert sharded == one
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29567"] + cmd, cwd=str(on),
                         env=_env(1, training=False, MACR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    assert _lines(two.stdout) == one, two.stdout                            # the main rank alone prints, and prints the same


def test_mf_tuner_prints_it_for_the_chosen_c_only(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    cmd = _mf_cmd(tmp_path, "tune.py") + ["--epoch", "2", "--start", "0", "--end", "1", "--step", "3", "--save_flag", "0"]
    out = _run(cmd, str(tmp_path), 1)
    assert sum(l.startswith("c:") for l in out.splitlines()) == 6 and len(_lines(out)) == 2, out      # 3 values of c, 2 evaluations
    assert all(re.fullmatch(LINE, l) for l in _lines(out)), _lines(out)


LGCN_FLAGS = ["--dataset", "tiny_data", "--verbose", "1", "--layer_size", "[64,64]", "--Ks", "[5, 10]", "--lr", "0.01", "--batch_size", "16",
              "--gpu_id", "0", "--log_interval", "1", "--saveID", "d", "--loss", "bceboth", "--test", "rubiboth", "--c", "0.5"]


def test_lightgcn_cli_calibration_report(ops, tmp_path):
    from macr_amd.data import LGCNData
    from macr_amd.lightgcn import LightGCN
    on = tmp_path / "on"
    shutil.copytree(os.path.join(GOLD, "tiny_data"), on / "data" / "tiny_data")
    flags = ["--data_path", str(on / "data") + "/", "--weights_path", str(on) + "/", "--epoch", "3"] + LGCN_FLAGS
    out2 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags, str(on), 2)
    lines = _lines(out2)
    assert len(lines) == 3, out2                                            # one per evaluation
    args = _load(os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"), "lgcn_parser_for_calibration").parse_args(flags)
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
    want, _ = _recomputed_line(here, base, train, test, data.n_items, counts, K)
    assert lines[-1] == want
    assert re.fullmatch(LINE + BASE, lines[-1]), lines[-1]
    value1, _ = _recomputed_line(here, None, train, test, data.n_items, counts, K)
    assert lines[-1].startswith(value1 + " | normal: ")


def test_lightgcn_tuner_prints_it_for_the_chosen_c_only(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    flags = ["--data_path", str(tmp_path / "data") + "/", "--weights_path", str(tmp_path) + "/", "--epoch", "2", "--start", "0", "--end", "1",
             "--step", "3"] + LGCN_FLAGS
    out = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN_tune.py")] + flags, str(tmp_path), 1)
    assert sum(l.startswith("c:") for l in out.splitlines()) == 6 and len(_lines(out)) == 2, out      # 3 values of c, 2 evaluations
    assert all(re.fullmatch(LINE, l) for l in _lines(out)), _lines(out)
