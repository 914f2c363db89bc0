"""The host half of MACR_CALIBRATION_REPORT (macr_amd/calibration.py) against the plain-loop restatement
(tests/calibration_ref.py), and macr_group_hist's bindings and refusals through the C ABI -- all without a GPU.  Counts and tv
are compared exactly; float figures at 1e-12 absolute: each is at most 2 * 64 correctly rounded terms of magnitude <= 1
(the test's train counts stay below 1000, so a mean popularity is off by less than 2 ulp(1000) = 2.3e-13)."""
import ctypes
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import calibration_ref as R
from macr_amd import _lib, calibration
from macr_amd.build import build

TOL = 1e-12
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b):
    return (a != a and b != b) or abs(a - b) <= TOL


def same_report(got, want):
    for key in ("users", "k", "skipped"):
        if key in want:
            assert got[key] == want[key], key
    for key in ("js", "tv", "gap_profile", "gap_list", "lift", "recall"):
        assert close(got[key], want[key]), (key, got[key], want[key])
    for t in R.TASTE:
        assert got["taste"][t]["users"] == want["taste"][t]["users"], t
        for key in ("js", "tv", "gap_profile", "gap_list", "lift", "recall"):
            assert close(got["taste"][t][key], want["taste"][t][key]), (t, key, got["taste"][t][key], want["taste"][t][key])


def make_counts(seed, U, n_groups=6, k=20):
    """(profile, here, base, gt_sizes) as the device leaves them, by the restatement's kernel on random rows: user 3 has no
    train list, user 5 an all -1 list; the train counts stay below 1000"""
    rs = np.random.RandomState(seed)
    n_items = 400
    weight = rs.randint(1, 1000, n_items).astype(np.int32)
    group_of = np.minimum(weight // 170, n_groups - 1).astype(np.int32)
    train = [sorted(rs.choice(n_items, rs.randint(1, 60), replace=False).tolist()) for _ in range(U)]
    if U > 3:
        train[3] = []
    lists = [np.stack([rs.permutation(n_items)[:k] for _ in range(U)]).astype(np.int32) for _ in range(2)]
    if U > 5:
        lists[0][5] = -1
    gt = [sorted(set(rs.randint(0, n_items, rs.randint(0, 5)).tolist()) | set(lists[0][u, :rs.randint(0, 3)].tolist()) - {-1}) for u in range(U)]
    p_cnt, _, p_wsum = R.group_hist(train, group_of, n_groups, n_items, item_weight=weight)
    here, base = (R.group_hist(l, group_of, n_groups, n_items, gt, weight, k=k) for l in lists)
    return (p_cnt, p_wsum), here, base, np.array([len(g) for g in gt])


def test_js_is_0_for_equal_mixes_and_1_for_disjoint_ones():
    assert calibration.js([1, 2, 0, 4], [3, 6, 0, 12]) == 0.0
    assert calibration.js([7], [20]) == 0.0
    assert calibration.js([3, 0, 5, 0], [0, 2, 0, 9]) == 1.0
    assert calibration.js([1, 0], [0, 1]) == 1.0
    rs = np.random.RandomState(0)
    for _ in range(200):
        a, b = rs.randint(0, 30, 6), rs.randint(0, 30, 6)
        a[rs.randint(6)] += 1
        b[rs.randint(6)] += 1
        v = calibration.js(a, b)
        assert 0.0 <= v <= 1.0 and close(v, R.js(a, b)) and close(v, calibration.js(b, a))
    # 64 groups, large counts
    a, b = rs.randint(0, 2 ** 31 - 1, 64), rs.randint(0, 2 ** 31 - 1, 64)
    assert close(calibration.js(a, b), R.js(a, b))
    with pytest.raises(ValueError):
        calibration.js([0, 0], [1, 2])


def test_tv_is_an_exact_rational():
    assert calibration.tv([1, 2, 3], [1, 2, 3]) == 0 and calibration.tv([5, 0], [0, 2]) == 1
    assert calibration.tv([1, 1, 1], [2, 1, 0]) == Fraction(1, 3)
    assert calibration.tv([1, 3], [1, 1]) == Fraction(1, 4)
    rs = np.random.RandomState(1)
    for _ in range(200):
        a, b = rs.randint(0, 2 ** 31 - 1, 64), rs.randint(0, 2 ** 31 - 1, 64)          # the numerator passes 2^63
        got = calibration.tv(a, b)
        assert isinstance(got, Fraction) and got == R.tv(a, b) and 0 <= got <= 1
    with pytest.raises(ValueError):
        calibration.tv([1, 2], [0, 0])


def test_taste_group_cuts_with_ties_and_few_users():
    assert calibration.taste_groups([]) == ([], [], [])
    for n in range(1, 5):                              # n < 5: floor(n / 5) = 0, everyone is diverse
        assert calibration.taste_groups(list(range(n, 0, -1))) == ([], list(range(n - 1, -1, -1)), [])
    assert calibration.taste_groups([5, 4, 3, 2, 1]) == ([4], [3, 2, 1], [0])
    # ties: the position in the user list decides, on both edges
    keys = [Fraction(2), Fraction(1), Fraction(1), Fraction(1), Fraction(2), Fraction(2), Fraction(1), Fraction(2), Fraction(2), Fraction(2)]
    assert calibration.taste_groups(keys) == ([1, 2], [3, 6, 0, 4, 5, 7], [8, 9])
    n, d, b = calibration.taste_groups([7] * 11)
    assert (n, d, b) == ([0, 1], list(range(2, 9)), [9, 10])
    rs = np.random.RandomState(2)
    keys = [Fraction(int(x), 3) for x in rs.randint(0, 8, 57)]
    want = R.taste_cuts(dict(enumerate(keys)))
    assert calibration.taste_groups(keys) == tuple(want) and [len(x) for x in want] == [11, 35, 11]


@pytest.mark.parametrize("U", [1, 4, 7, 60])
def test_summarize_against_the_restatement_with_skipped_users(U):
    profile, here, base, sizes = make_counts(U, U)
    for b in (None, base):
        got = calibration.summarize(profile, here, sizes, 20, b)
        want = R.summarize(profile, here, sizes, 20, b)
        same_report(got, want)
        if b is not None:
            same_report(got["base"], want["base"])
            assert got["base"]["users"] == got["users"]
        assert got["skipped"] == (U > 3) + (U > 5) and got["users"] == U - got["skipped"]
    if U == 60:
        rep = calibration.summarize(profile, here, sizes, 20)
        # 59 users with a profile are cut 11 / 37 / 11; the one of them without a list is counted in none
        assert [rep["taste"][t]["users"] for t in R.TASTE] in ([10, 37, 11], [11, 36, 11], [11, 37, 10])
        assert sum(rep["taste"][t]["users"] for t in R.TASTE) == rep["users"] == 58
        assert rep["taste"]["niche"]["gap_profile"] < rep["taste"]["diverse"]["gap_profile"] < rep["taste"]["blockbuster"]["gap_profile"]
        assert 0 < rep["js"] < 1 and 0 < rep["tv"] < 1 and rep["recall"] > 0


def test_everyone_skipped_gives_nan_and_a_line():
    p = (np.zeros((3, 6), dtype=np.int32), np.zeros((3, 2), dtype=np.int64))
    h = (np.ones((3, 6), dtype=np.int32), np.zeros((3, 6), dtype=np.int32), np.full((3, 2), 6, dtype=np.int64))
    rep = calibration.summarize(p, h, np.ones(3, dtype=np.int64), 20)
    assert rep["users"] == 0 and rep["skipped"] == 3 and math.isnan(rep["js"]) and math.isnan(rep["lift"])
    assert "users=0 skipped=3 js=nan" in calibration.format_line(rep)
    with pytest.raises(ValueError):
        calibration.summarize((p[0].astype(np.float32), p[1]), h, np.ones(3, dtype=np.int64), 20)


def test_the_line_is_identical_under_permuted_summation_order():
    """the means are math.fsum: what the line prints does not depend on the order the users are summed in.  Permuting the
    users keeps every set (the taste groups are cut by profile popularity; equal keys are avoided by distinct profiles)."""
    profile, here, base, sizes = make_counts(11, 60)
    keys = [Fraction(int(w), int(n)) for w, n in profile[1] if n > 0]
    assert len(set(keys)) == len(keys)
    line = calibration.format_line(calibration.summarize(profile, here, sizes, 20, base))
    rs = np.random.RandomState(5)
    for _ in range(5):
        perm = rs.permutation(60)
        pick = lambda t: tuple(x[perm] for x in t)
        assert calibration.format_line(calibration.summarize(pick(profile), pick(here), sizes[perm], 20, pick(base))) == line
    assert line.startswith("calibration @20: users=58 skipped=2 js=0.") and line.count(" | ") == 2
    assert "| users by profile popularity (niche 20%, diverse 60%, blockbuster 20%): users=[" in line and " | normal: js=0." in line
    one = calibration.format_line(calibration.summarize(profile, here, sizes, 20))
    assert line.startswith(one + " | normal: ")


def test_switch(monkeypatch):
    for value, want in ((None, 0), ("", 0), ("0", 0), ("1", 1), ("2", 2), ("3", 0), ("yes", 0)):
        if value is None:
            monkeypatch.delenv("MACR_CALIBRATION_REPORT", raising=False)
        else:
            monkeypatch.setenv("MACR_CALIBRATION_REPORT", value)
        assert calibration.enabled() == want
    assert "MACR_CALIBRATION_REPORT=2" in calibration.BASE_IS_THE_LIST


def test_host_half_needs_neither_torch_nor_the_library():
    code = ("import sys; import macr_amd.calibration as c; "
            "assert 'torch' not in sys.modules and 'macr_amd._lib' not in sys.modules and 'macr_amd.ops' not in sys.modules; "
            "print(c.enabled())")
    env = dict(os.environ, PYTHONPATH=REPO)
    env.pop("MACR_CALIBRATION_REPORT", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr[-2000:]


# ------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    build()
    return _lib.lib()


def test_binding_and_abi(lib):
    assert len(_lib.SIGNATURES["macr_group_hist"][1]) == 15
    assert _lib.ABI_VERSION == 16 and lib.macr_abi_version() == 16
    assert hasattr(lib, "macr_group_hist") and "macr_group_hist" not in _lib.TEST_SIGNATURES
    header = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    assert "int macr_group_hist(int U, const int32_t *row_ptr, const int32_t *ids, int stride, int k," in header
    assert "macr_group_hist" not in open(os.path.join(REPO, "include", "macr_hip_test.h")).read()


def test_refusals_come_before_any_device_work(lib):
    """every refusal of the header, through the C ABI on host pointers that are never dereferenced"""
    buf = ctypes.create_string_buffer(256)
    base = ctypes.cast(buf, ctypes.c_void_p).value
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)
    # U, row_ptr, ids, stride, k, gt_ptr, gt_idx, n_items, group_of, n_groups, item_weight, cnt, hit, wsum, stream
    ok = dict(U=4, row_ptr=None, ids=p, stride=32, k=20, gt_ptr=p, gt_idx=p, n_items=100, group_of=p, n_groups=6,
              item_weight=p, cnt=p, hit=p, wsum=p)
    order = list(ok)
    cases = [(dict(U=0), b"U=0"), (dict(U=-2), b"U=-2"), (dict(n_items=0), b"n_items=0"), (dict(n_items=-5), b"n_items=-5"),
             (dict(n_groups=0), b"n_groups=0"), (dict(n_groups=65), b"n_groups=65"), (dict(n_groups=-1), b"n_groups=-1"),
             (dict(ids=None), b"ids"), (dict(group_of=None), b"group_of"), (dict(cnt=None), b"cnt"),
             (dict(k=0), b"k=0"), (dict(k=-1), b"k=-1"), (dict(k=33), b"k=33"), (dict(stride=0, k=1), b"stride=0"),
             (dict(row_ptr=p), b"stride=32"), (dict(row_ptr=p, stride=0), b"k=20"), (dict(row_ptr=p, k=0), b"stride=32"),
             (dict(hit=None), b"hit"), (dict(gt_ptr=None), b"gt_ptr"), (dict(gt_idx=None), b"gt_idx"),
             (dict(hit=None, gt_ptr=None), b"gt_idx"), (dict(gt_ptr=None, gt_idx=None), b"hit"),
             (dict(wsum=odd), b"wsum")]
    for change, word in cases:
        args = dict(ok, **change)
        rc = lib.macr_group_hist(*[args[name] for name in order], None)
        err = lib.macr_last_error()
        assert rc == _lib.E_INVALID and b"group_hist" in err and word in err, (change, err)
