"""Per-item accuracy diagnostic (--out 1), host side: the NumPy restatement (tests/item_acc_ref.py) against what the
reference's two test() functions computed (G15, tests/golden/make_golden_item_acc.py), macr_amd/popularity.py against the
restatement, and the argument refusals of macr_item_counts (which come before any device work, so need no GPU)."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

import item_acc_ref as R
from helpers import GOLD, REPO, dataset_args, score_matrix

from macr_amd import _lib, popularity
from macr_amd.data import LGCNData, MFData


@pytest.fixture(scope="module")
def g15():
    return json.load(open(os.path.join(GOLD, "G15_item_acc.json")))


@pytest.mark.parametrize("kind", ["normal", "popular"])
def test_restatement_equals_the_reference_mf_dictionary(g15, kind):
    data = MFData(dataset_args("tiny"))
    users = list(data.test_user_list.keys())
    full = score_matrix(kind, data.n_users, data.n_items, g15["seeds"][kind])
    train, test = data.eval_lists(users)
    rec, hit, n_test, d = R.item_accuracy(full[users], train, test, g15["k"]["mf"])
    assert str(d) == g15["mf"][kind]
    assert np.array_equal(n_test, [len(data.test_item_list[i]) for i in range(data.n_items)])
    assert str(popularity.item_acc_dict(hit, n_test)) == g15["mf"][kind]


@pytest.mark.parametrize("kind", ["normal", "popular"])
def test_restatement_equals_the_reference_lightgcn_file(g15, kind):
    args = dataset_args("tiny")
    data = LGCNData(args.data_path + args.dataset, args.batch_size, args)
    users = list(data.test_set.keys())
    full = score_matrix(kind, data.n_users, data.n_items, g15["seeds"][kind])
    train, test = data.eval_lists(users)
    rec, hit, n_test, d = R.item_accuracy(full[users], train, test, g15["k"]["lgcn"])
    assert str(d) == g15["lgcn"][kind]
    assert np.array_equal(n_test, [len(data.test_item_set[i]) for i in range(data.n_items)])
    assert str(popularity.item_acc_dict(hit, n_test)) == g15["lgcn"][kind]
    assert rec.sum() == sum(min(20, data.n_items - len(t)) for t in train)      # every candidate slot filled and counted


def test_item_groups_at_the_cut_points():
    counts = [0, 10, 11, 50, 51, 500, 501, 1, 100, 101, 200, 201]
    want = [0, 0, 1, 1, 2, 4, 5, 0, 2, 3, 3, 4]
    assert popularity.item_groups(counts).tolist() == want
    assert R.groups_of(counts).tolist() == want
    assert popularity.item_groups([3, 4, 5], points=(3, 4)).tolist() == [0, 1, 2]


def test_item_groups_of_addressa_and_of_plot_pics():
    data = MFData(dataset_args("addressa"))
    counts = popularity.train_counts(data.train_item_list, data.n_items)
    group_of = popularity.item_groups(counts)
    assert np.bincount(group_of, minlength=6).tolist() == [370, 223, 32, 16, 42, 61]
    assert np.array_equal(group_of, R.groups_of(counts))
    # the `belong` / `sorted_id` globals of macr_mf/batch_test.py name the same groups (items with train interactions)
    sorted_id, belong = data.plot_pics()[:2]
    keys = np.asarray(list(data.train_item_list.keys()))
    assert np.array_equal(group_of[keys[sorted_id]], belong)


def test_item_acc_dict_is_the_repeated_add_form():
    for n in range(1, 8):
        hit = np.arange(0, 8)
        d = popularity.item_acc_dict(hit, np.full(8, n))
        want = R.acc_dict(hit, np.full(8, n))
        assert str(d) == str(want)
        assert d[0] == 0 and isinstance(d[0], int)
        assert all(isinstance(d[h], float) for h in range(1, 8))
    assert str(popularity.item_acc_dict([6], [7])) != str({0: 6 / 7})        # the form matters: 0.857142857142857
    with pytest.raises(ValueError):
        popularity.item_acc_dict([1], [0])


def test_group_report_equals_the_restatement_table():
    rs = np.random.RandomState(3)
    n = 200
    group_of = popularity.item_groups(rs.randint(0, 700, n))
    n_test = rs.randint(0, 5, n)
    rec = rs.randint(0, 50, n)
    hit = np.minimum(rec, rs.randint(0, 3, n)) * (n_test > 0)
    hit = np.minimum(hit, n_test)
    got = popularity.group_report(group_of, rec, hit, n_test)
    want = R.group_table(group_of, rec, hit, n_test)
    assert [r.keys() for r in got] == [r.keys() for r in want]
    for a, b in zip(got, want):
        for key in a:
            assert a[key] == pytest.approx(b[key], rel=1e-12, abs=0), key
    assert popularity.group_report(group_of, rec, hit, n_test, group_sums=R.group_sums(group_of, rec, hit, 6)) == got
    line = popularity.format_report(got, 5)
    assert line.startswith("item groups @5: catalogue=[") and line.count(",") == 15


def test_item_counts_refuses_bad_arguments_before_any_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)            # never dereferenced: every call below is refused on its arguments

    def call(U=4, K=20, k=5, rankings=p, gt_ptr=p, gt_idx=p, n_items=10, group_of=None, n_groups=0, rec=p, hit=p, out=None,
             ws=p, ws_bytes=1 << 30):
        return L.macr_item_counts(U, K, k, rankings, gt_ptr, gt_idx, n_items, group_of, n_groups, rec, hit, out, ws, ws_bytes, None)

    bad = [dict(k=0), dict(k=-1), dict(k=21), dict(K=5, k=6), dict(n_items=0), dict(n_items=-3), dict(rankings=None),
           dict(gt_ptr=None), dict(gt_idx=None), dict(rec=None), dict(hit=None), dict(group_of=p, n_groups=0),
           dict(group_of=p, n_groups=65), dict(group_of=p, n_groups=-1, out=p), dict(U=0), dict(ws=None),
           dict(ws=ctypes.c_void_p(0x1004)), dict(k=0, ws=None, ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"item_counts" in L.macr_last_error(), kw
    need = L.macr_item_counts_workspace_bytes(4, 20, 10)
    assert need > 0 and need % 8 == 0
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE and b"workspace" in L.macr_last_error()
    assert call(k=0, ws_bytes=0) == _lib.E_INVALID             # the arguments are judged before the workspace's size
    assert "macr_item_counts" in _lib.SIGNATURES and "macr_item_counts_workspace_bytes" in _lib.SIGNATURES


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("path, file", [("macr_mf/parse.py", "MF_macr.txt"), ("macr_lightgcn/utility/parser.py", "Lightgcn_macr.txt")])
def test_out_flag_help_names_the_diagnostic(path, file):
    mod = _load(os.path.join(REPO, path), "cli_parser_" + file[:2])
    text = " ".join(mod.build_parser().format_help().split())
    assert "per-item accuracy diagnostic" in text and file in text
    assert mod.parse_args([]).out == 0
