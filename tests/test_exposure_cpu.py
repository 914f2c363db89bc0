"""Exposure report (MACR_EXPOSURE_REPORT=1), host side: macr_amd/exposure.py against the restatement (tests/exposure_ref.py)
and known answers, and the declaration, binding and argument refusals of macr_item_exposure (which come before any device
work, so need no GPU)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import exposure_ref as R
from helpers import REPO

from macr_amd import _lib, exposure


def test_entry_points_are_declared_bound_and_exported_at_abi_16():
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in ("macr_item_exposure", "macr_item_exposure_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.ABI_VERSION == 16 == L.macr_abi_version()
    assert re.search(r"#define MACR_ABI_VERSION\s+16\b", src)
    # the kernel's constants: the header's are the binding's
    consts = dict(re.findall(r"#define (MACR_ITEM_EXPOSURE_[A-Z_]+)\s+(\d+)", src))
    assert {k: int(v) for k, v in consts.items()} == {
        "MACR_ITEM_EXPOSURE_BINS": _lib.ITEM_EXPOSURE_BINS, "MACR_ITEM_EXPOSURE_TILE": _lib.ITEM_EXPOSURE_TILE,
        "MACR_ITEM_EXPOSURE_MAX_BLOCKS": _lib.ITEM_EXPOSURE_MAX_BLOCKS, "MACR_ITEM_EXPOSURE_REPLICAS": _lib.ITEM_EXPOSURE_REPLICAS}
    # two 64-bit counters per item and copy
    assert L.macr_item_exposure_workspace_bytes(4, 20, 10) == _lib.ITEM_EXPOSURE_REPLICAS * 10 * 16


def test_item_exposure_refuses_bad_arguments_before_any_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)            # never dereferenced: every call below is refused on its arguments

    def call(U=4, K=20, k=5, rankings=p, gt_ptr=p, gt_idx=p, weight=p, n_items=10, group_of=None, n_groups=0, exp_w=p, hit_w=p,
             out=None, ws=p, ws_bytes=1 << 30):
        return L.macr_item_exposure(U, K, k, rankings, gt_ptr, gt_idx, weight, n_items, group_of, n_groups, exp_w, hit_w, out,
                                    ws, ws_bytes, None)

    bad = [dict(U=0), dict(U=-2), dict(k=0), dict(k=-1), dict(k=21), dict(K=5, k=6), dict(n_items=0), dict(n_items=-3),
           dict(rankings=None), dict(gt_ptr=None), dict(gt_idx=None), dict(weight=None), dict(exp_w=None), dict(hit_w=None),
           dict(group_of=p, n_groups=0), dict(group_of=p, n_groups=65), dict(group_of=p, n_groups=-1, out=p), dict(ws=None),
           dict(ws=ctypes.c_void_p(0x1004)), dict(k=0, ws=None, ws_bytes=0)]
    for kw in bad:
        assert call(**kw) == _lib.E_INVALID, kw
        assert b"item_exposure" in L.macr_last_error(), kw
    need = L.macr_item_exposure_workspace_bytes(4, 20, 10)
    assert need > 0 and need % 16 == 0
    assert call(ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert b"item_exposure" in L.macr_last_error() and b"workspace" in L.macr_last_error()
    assert call(k=0, ws_bytes=0) == _lib.E_INVALID             # the arguments are judged before the workspace's size
    assert call(weight=None, ws_bytes=0) == _lib.E_INVALID
    assert L.macr_item_exposure_workspace_bytes(0, 20, 10) == 0 and L.macr_item_exposure_workspace_bytes(4, 20, 0) == 0


def test_position_weights():
    w = exposure.position_weights(128)
    assert w.dtype == np.uint32 and w.shape == (128,)
    assert int(w[0]) == 2 ** 24
    assert int(w[1]) == math.floor(2 ** 24 / math.log2(3) + 0.5) == 10585245
    assert int(w[2]) == 2 ** 23                                  # 1 / log2(4)
    assert np.all(np.diff(w.astype(np.int64)) < 0)               # strictly decreasing
    assert np.array_equal(w, R.weights(128))
    assert np.array_equal(exposure.position_weights(1), [2 ** 24])
    with pytest.raises(ValueError):
        exposure.position_weights(0)


def test_gini_known_answers():
    assert exposure.gini([5, 5, 5, 5]) == 0.0
    assert exposure.gini(np.full(1000, 3, dtype=np.int32)) == 0.0
    for n in (1, 2, 7, 1000):
        x = np.zeros(n, dtype=np.int64)
        x[n // 2] = 12345
        assert exposure.gini(x) == (n - 1) / n, n
    assert math.isnan(exposure.gini([0, 0, 0])) and math.isnan(exposure.gini(np.zeros(9, dtype=np.int32)))
    assert exposure.gini([0, 1, 1, 2]) == 0.375                 # (-3*0 - 1 + 1 + 3*2) / (4 * 4)
    rs = np.random.RandomState(0)
    x = rs.randint(0, 1 << 40, 500).astype(np.int64) * (rs.random_sample(500) < 0.6)
    g = exposure.gini(x)
    assert 0.0 < g < 1.0 and g == R.gini(x)
    for _ in range(3):
        assert exposure.gini(rs.permutation(x)) == g             # a function of the multiset
    # sums past 2^63 in the numerator: exact integers all the way
    big = np.array([0, 0, (1 << 62) - 1, 1 << 62], dtype=np.int64)
    assert exposure.gini(big) == R.gini(big)


def test_summarize_equals_the_restatement():
    rs = np.random.RandomState(11)
    for n, n_groups in ((1, 1), (17, 6), (400, 6), (400, 64)):
        for trial in range(3):
            rec = rs.randint(0, 50, n) * (rs.random_sample(n) < 0.7)
            exp_w = rec.astype(np.int64) * rs.randint(1 << 20, 1 << 24, n)
            hit_w = (exp_w * (rs.random_sample(n) < 0.3)) // rs.randint(1, 4, n)
            if trial == 2:
                hit_w[:] = 0                                     # no hit at all: the dcg shares are nan
            train = rs.randint(0, 900, n)
            group_of = rs.randint(-1, n_groups + 1, n)           # some items outside every group
            got = exposure.summarize(rec.astype(np.int32), exp_w, hit_w, train, group_of, n_groups, 33, 20)
            want = R.summarize(rec, exp_w, hit_w, train, group_of, n_groups, 33, 20)
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), (n, n_groups, trial, key)
            assert exposure.format_line(got) == R.format_line(want)
    empty = exposure.summarize(np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64), [1] * 5,
                               [0] * 5, 6, 0, 20)
    assert empty["slots"] == 0 and empty["coverage"] == 0.0
    assert all(math.isnan(empty[key]) for key in ("gini", "gini_dcg", "arp", "arp_dcg"))
    assert np.isnan(empty["group_exposure"]).all() and np.isnan(empty["group_dcg_hits"]).all()


def test_hand_computed_line():
    """2 users, k = 2, 4 items: lists [0, 1] and [0, 2], ground truths {1} and {0}; W0 = 2^24, W1 = 10585245 = 0.63093 W0.
    rec = [2, 1, 1, 0]: slots 4, coverage 3/4, gini 6/16, arp (2*100 + 5 + 20) / 4 = 56.25
    exp = [2 W0, W1, W1, 0]: gini_dcg = 6 W0 / (8 (W0 + W1)) = 0.45986, arp_dcg = (200 W0 + 25 W1) / (2 W0 + 2 W1) = 66.15
    train counts [100, 5, 20, 1] -> groups [2, 0, 1, 0]: exposure shares W1 / (2 W0 + 2 W1) = 0.19343 (twice) and
    W0 / (W0 + W1) = 0.61315; hits = [W0, W1, 0, 0]: shares W1 / (W0 + W1) = 0.38685, 0, 0.61315"""
    from macr_amd import popularity
    W0, W1 = (int(v) for v in exposure.position_weights(2))
    train = [100, 5, 20, 1]
    group_of = popularity.item_groups(train)
    assert group_of.tolist() == [2, 0, 1, 0]
    rep = exposure.summarize([2, 1, 1, 0], [2 * W0, W1, W1, 0], [W0, W1, 0, 0], train, group_of, 6, 2, 2)
    assert exposure.format_line(rep) == (
        "exposure @2: users=2 slots=4 coverage=0.75000 gini=0.37500 gini_dcg=0.45986 arp=56.25 arp_dcg=66.15 | "
        "train-popularity groups (<10,<50,<100,<200,<500,>=500): "
        "exposure=[0.19343, 0.19343, 0.61315, 0.00000, 0.00000, 0.00000] "
        "dcg_hits=[0.38685, 0.00000, 0.61315, 0.00000, 0.00000, 0.00000]")


def test_enabled_follows_the_variable(monkeypatch):
    monkeypatch.delenv("MACR_EXPOSURE_REPORT", raising=False)
    assert exposure.enabled() is False
    for value, want in (("", False), ("0", False), ("1", True), ("true", False)):
        monkeypatch.setenv("MACR_EXPOSURE_REPORT", value)
        assert exposure.enabled() is want, value


def test_the_switch_is_no_parser_flag():
    for path in ("macr_mf/parse.py", "macr_lightgcn/utility/parser.py"):
        text = open(os.path.join(REPO, path)).read()
        assert "EXPOSURE" not in text.upper(), path
    for path in ("macr_mf/train.py", "macr_lightgcn/utility/branch_ranking.py", "macr_lightgcn/LightGCN.py"):
        assert "exposure.enabled()" in open(os.path.join(REPO, path)).read(), path


def test_exposure_module_needs_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import macr_amd.exposure as e; "
            "assert 'torch' not in sys.modules and 'macr_amd._lib' not in sys.modules; "
            "print(int(e.position_weights(3)[2]))" % REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == str(2 ** 23), out.stderr[-2000:]
