"""The list shift report (MACR_SHIFT_REPORT), host side: the restatement (tests/shift_ref.py) on hand-worked lists, and
macr_amd/shift_report.py -- the exact sign test against brute-force binomial sums, totals past 2^31, the all-identical input,
the line's format and the parse of the variable.  No GPU."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import shift_ref as R
from macr_amd import shift_report as S


# ----------------------------------------------------------------------------- the restatement, by hand
def test_ref_hand_worked_rows():
    #            base                 here                  truth
    rows = [([5, 3, 9, 1], [3, 5, 7, 1], [1, 7, 9]),         # swap at the top, 9 left (lost hit), 7 entered (gained hit), 1 kept
            ([4, 2, -1, -1], [4, 2, -1, -1], []),            # identical, -1 tails, empty truth
            ([0, 1, 2, 3], [3, 2, 1, 0], [0]),               # the same set reversed
            ([0, 1, 2, 3], [6, 7, 8, 9], [2, 8, 9]),         # disjoint
            ([-1, -1, -1, -1], [2, 11, -1, 5], [2]),         # empty base; 11 >= n_items is skipped
            ([7, -1, 4, 10], [7, 4, -1, 12], [4])]           # -1 in the middle; ids >= n_items differ as raw slots only
    base, here, gt = (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), [r[2] for r in rows])
    pu, ent, left = R.list_shift(base, here, gt, 4, 10)
    assert pu.dtype == ent.dtype == left.dtype == np.int32
    assert pu.tolist() == [[4, 4, 3, 0, 2, 2, 2, 1],
                           [2, 2, 2, 4, 0, 0, 0, 0],
                           [4, 4, 4, 0, 8, 1, 1, 1],
                           [4, 4, 0, 0, 0, 1, 2, 0],
                           [0, 2, 0, 0, 0, 0, 1, 0],
                           [2, 2, 2, 1, 1, 1, 1, 1]]
    assert ent.tolist() == [[7, -1, -1, -1], [-1] * 4, [-1] * 4, [6, 7, 8, 9], [2, 5, -1, -1], [-1] * 4]
    assert left.tolist() == [[9, -1, -1, -1], [-1] * 4, [-1] * 4, [0, 1, 2, 3], [-1] * 4, [-1] * 4]
    # only the first k slots count
    pu2, ent2, _ = R.list_shift(base, here, gt, 2, 10)
    assert pu2[0].tolist() == [2, 2, 2, 0, 2, 0, 0, 0] and ent2.shape == (6, 2) and ent2[3].tolist() == [6, 7]
    ptr, idx = R.pairs_of(ent)
    assert ptr.tolist() == [0, 1, 1, 1, 5, 7, 7] and idx.tolist() == [7, 6, 7, 8, 9, 2, 5]


def test_ref_refuses_a_repeated_id():
    with pytest.raises(AssertionError):
        R.list_shift(np.array([[1, 1]]), np.array([[1, 2]]), [[]], 2, 5)


def test_ref_full_positions():
    scores = np.array([[0.5, 0.9, 0.5, 0.1, 0.7]], dtype=np.float32)
    # candidates outside train {4}: 1 (0.9), 0 (0.5), 2 (0.5, tie by id), 3 (0.1)
    assert R.full_positions(scores, [[4]], np.array([[2, 3, -1, 4, 1]])).tolist() == [2, 3, -1, 0]


# ----------------------------------------------------------------------------- the sign test
def _pascal(n):
    row = [1]
    for _ in range(n):
        row = [1] + [row[i] + row[i + 1] for i in range(len(row) - 1)] + [1]
    return row


def test_sign_test_against_brute_force_binomial_sums():
    assert S.sign_test(0, 0) == 1
    for better in range(13):
        for worse in range(13 - better):
            n, m = better + worse, min(better, worse)
            row = _pascal(n)
            want = min(Fraction(1), 2 * sum(Fraction(row[i], 2 ** n) for i in range(m + 1)))
            got = S.sign_test(better, worse)
            assert isinstance(got, Fraction) and got == want, (better, worse)
            assert got == S.sign_test(worse, better)
    assert S.sign_test(5, 5) == 1 and S.sign_test(0, 1) == 1 and S.sign_test(0, 2) == Fraction(1, 2)
    assert S.sign_test(0, 10) == Fraction(2, 1024) and S.sign_test(3, 9) == Fraction(2 * (1 + 12 + 66 + 220), 4096)
    # far past float range of 2^n: still exact, and the float of it underflows to a number, not an error
    big = S.sign_test(100, 3000)
    assert big == Fraction(2 * sum(math.comb(3100, i) for i in range(101)), 2 ** 3100) and 0.0 <= float(big) < 1e-300
    with pytest.raises(ValueError):
        S.sign_test(-1, 2)


# ----------------------------------------------------------------------------- summarize / format_line
def _counts(ent, left, pu_gt, n_items):
    """per-item (rec, hit) of the entered and left lists, by plain loops"""
    out = []
    for ids in (ent, left):
        rec, hit = np.zeros(n_items, dtype=np.int64), np.zeros(n_items, dtype=np.int64)
        for u, row in enumerate(ids):
            for i in row:
                if i >= 0:
                    rec[i] += 1
                    hit[i] += int(i in pu_gt[u])
        out += [rec, hit]
    return out


def test_summarize_on_the_hand_worked_rows():
    base = np.array([[5, 3, 9, 1], [4, 2, -1, -1], [0, 1, 2, 3], [0, 1, 2, 3]])
    here = np.array([[3, 5, 7, 1], [4, 2, -1, -1], [3, 2, 1, 0], [6, 7, 8, 9]])
    gt = [[1, 7, 9], [], [0], [2, 8, 9]]
    pu, ent, left = R.list_shift(base, here, gt, 4, 10)
    group_of = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5])
    rep = S.summarize(pu, *_counts(ent, left, gt, 10), group_of, 6, 4)
    assert (rep["users"], rep["k"], rep["identical"]) == (4, 4, 1)
    assert rep["overlap"] == (3 + 2 + 4 + 0) / 14 and rep["first_diff"] == (0 + 4 + 0 + 0) / 4 and rep["footrule"] == (2 + 0 + 8) / 9
    assert (rep["hits_base"], rep["hits_here"], rep["kept"], rep["gained"], rep["lost"]) == (4, 5, 2, 3, 2)
    assert (rep["better"], rep["worse"], rep["sign_p"]) == (1, 0, 1.0)
    assert rep["group_entered"].tolist() == [0, 0, 0, 3 / 5, 1 / 5, 1 / 5] and rep["group_left"].tolist() == [2 / 5, 2 / 5, 0, 0, 0, 1 / 5]
    assert rep["group_gained"].tolist() == [0, 0, 0, 1, 1, 1] and rep["group_lost"].tolist() == [0, 1, 0, 0, 0, 1]
    assert rep["group_gained"].sum() == rep["gained"] and rep["group_lost"].sum() == rep["lost"]
    line = S.format_line(rep)
    assert line == ("shift @4 vs normal: users=4 identical=1 overlap=0.64286 first_diff=1.000 footrule=1.111 | "
                    "hits base=4 here=5 kept=2 gained=3 lost=2 users better=1 worse=0 sign_p=1 | "
                    "train-popularity groups (<10,<50,<100,<200,<500,>=500): entered=[0.00000, 0.00000, 0.00000, 0.60000, 0.20000, 0.20000] "
                    "left=[0.40000, 0.40000, 0.00000, 0.00000, 0.00000, 0.20000] gained=[0, 0, 0, 1, 1, 1] lost=[0, 1, 0, 0, 0, 1]")
    assert "depth" not in line
    deep = S.format_line(S.summarize(pu, *_counts(ent, left, gt, 10), group_of, 6, 4,
                                     depth=(np.array([9, 4, -1, 30, 7]), np.array([-1, -1]))))
    assert deep == line + " | depth: entered med=7 p90=30 max=30 left med=nan p90=nan max=nan (skipped=3)"


def test_depth_quantiles_are_nearest_rank():
    d = S.summarize_depth(np.arange(10)[::-1], np.array([5], dtype=np.int32))
    assert d == {"entered": (4, 8, 9), "left": (5, 5, 5), "skipped": 0}
    d = S.summarize_depth(np.array([-1, 3, 3, 100]), np.array([], dtype=np.int64))
    assert d == {"entered": (3, 100, 100), "left": (None, None, None), "skipped": 1}


def test_totals_pass_2_31():
    U, k = 3000, 128
    pu = np.zeros((U, 8), dtype=np.int32)
    pu[:, 0] = pu[:, 1] = pu[:, 2] = k
    pu[:, 3] = k
    pu[:, 4] = k * k // 2                      # the footrule of a reversed row of 128: 8192 per user
    pu[:, 4] = 2 ** 30                         # and far beyond: three users already pass 2^31
    pu[:, 5] = pu[:, 6] = pu[:, 7] = 2 ** 30
    zeros = np.zeros(5, dtype=np.int32)
    rep = S.summarize(pu, zeros, zeros, zeros, zeros, np.zeros(5, dtype=np.int32), 6, k)
    assert rep["hits_base"] == rep["hits_here"] == rep["kept"] == U * 2 ** 30 > 2 ** 31
    assert (rep["gained"], rep["lost"], rep["better"], rep["worse"]) == (0, 0, 0, 0)
    assert rep["footrule"] == (U * 2 ** 30) / (U * k) and rep["overlap"] == 1.0 and rep["identical"] == U
    assert "kept=%d " % (U * 2 ** 30) in S.format_line(rep)
    # int32 item counts whose SUM passes 2^31
    big = np.full(5, 2 ** 30, dtype=np.int32)
    rep = S.summarize(pu, big, zeros, big, zeros, np.array([0, 0, 0, 1, 7], dtype=np.int32), 6, k)
    assert rep["group_entered"].tolist() == [3 / 5, 1 / 5, 0, 0, 0, 0]              # (group 7 is in no group)


def test_all_identical_input():
    base = np.array([[3, 1, 4], [1, 5, -1]])
    pu, ent, left = R.list_shift(base, base.copy(), [[1], [9]], 3, 10)
    assert (ent == -1).all() and (left == -1).all()
    zeros = np.zeros(10, dtype=np.int32)
    rep = S.summarize(pu, zeros, zeros, zeros, zeros, np.zeros(10, dtype=np.int32), 6, 3)
    assert rep["identical"] == 2 and rep["overlap"] == 1.0 and rep["footrule"] == 0.0 and rep["first_diff"] == 3.0
    assert (rep["gained"], rep["lost"], rep["kept"], rep["sign_p"]) == (0, 0, 1, 1.0)
    assert all(math.isnan(v) for v in rep["group_entered"]) and all(math.isnan(v) for v in rep["group_left"])
    assert "entered=[nan, nan, nan, nan, nan, nan]" in S.format_line(rep) and "identical=2 overlap=1.00000" in S.format_line(rep)


def test_summarize_refuses_floats_and_wrong_shapes():
    z = np.zeros(4, dtype=np.int32)
    with pytest.raises(ValueError):
        S.summarize(np.zeros((2, 8)), z, z, z, z, z, 6, 3)
    with pytest.raises(ValueError):
        S.summarize(np.zeros((2, 7), dtype=np.int32), z, z, z, z, z, 6, 3)
    with pytest.raises(ValueError):
        S.summarize(np.zeros((2, 8), dtype=np.int32), z, z[:3], z, z, z, 6, 3)


def test_enabled(monkeypatch):
    monkeypatch.delenv("MACR_SHIFT_REPORT", raising=False)
    assert S.enabled() == 0
    for value, want in (("0", 0), ("1", 1), ("2", 2), ("", 0), ("3", 0), ("yes", 0), (" 1", 0), ("-1", 0)):
        monkeypatch.setenv("MACR_SHIFT_REPORT", value)
        assert S.enabled() == want, value


def test_refusal_and_notice_name_the_variable():
    assert "MACR_SHIFT_REPORT=2" in S.refusal("--row_shard 1") and "MACR_SHIFT_REPORT=1" in S.refusal("--row_shard 1")
    assert "--row_shard 1" in S.refusal("--row_shard 1") and "--test normal" in S.NOTHING_TO_COMPARE
    assert re.match(r"MACR_SHIFT_REPORT", S.NOTHING_TO_COMPARE)
