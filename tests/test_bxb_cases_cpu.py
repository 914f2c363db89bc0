"""Preconditions of the (B,B) form-choice cases (tests/bxb_cases.py), without a GPU: every case holds the waves, flag counts and
edge values its GPU test (tests/test_gpu_bxb_forms.py) is there for, by the oracle's own fp32 forward scalars and the numpy
restatement of the launch's decisions; the oracle alone stays within a third of that test's tolerances of the float64
restatement of the loss graph; and no edge or neutralised column is so light that losing it or counting it twice would pass.

The oracle hands out its derivatives through the gradient rows only (deu, dei, dej, dw, dwu: with u, i, j free of repeats these
ARE the rows of the tables' gradients the GPU test compares): they are held to the float64 rows directly, and dp, dn and the
derivatives by si, sj (da, db times the sigmoid's slope, plus the item term) are read back out of them by least squares."""
import functools

import numpy as np
import pytest

import bxb_cases as bc
import oracle


@functools.lru_cache(maxsize=None)
def _views(name):
    c = bc.case(name)
    fwd = bc.oracle_forward(c)
    ref = bc.f64_reference(c["kind"], c["u"], c["i"], c["j"], c["P"], c["Q"], c["w"], c["wu"])
    return c, fwd, ref


def _groups(cls):
    real = np.flatnonzero(cls["real"])
    return real[real % 2 == 0], real[real % 2 == 1]


def _near(x, want):
    return abs(float(x) - want) <= 2e-3 * abs(want)           # (the edges sit 5e-3 off their thresholds)


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_edge_columns_are_few_and_every_target_is_met(name):
    c, fwd, _ = _views(name)
    B = c["B"]
    assert len(c["cols"]) * 16 <= B
    assert len(set(c["u"])) == B and len(set(c["i"]) | set(c["j"])) == 2 * B          # each gradient row isolates one column
    ev = bc._edge_values(bc.Y_LO_PAIRS if c["R"] >= 2 else bc.Y_LO_SINGLE)
    for col, v in c["cols"].items():
        tp, tn = (v, np.nan) if c["layout"] == "a1" else ev[v]
        assert np.isnan(tp) or abs(fwd["p"][col] - tp) <= 1e-4 * abs(tp), (col, v, fwd["p"][col])
        assert np.isnan(tn) or abs(fwd["n"][col] - tn) <= 1e-4 * abs(tn), (col, v, fwd["n"][col])
    cls = fwd["cls"]
    level = 1.0 if c["layout"] == "a1" else None
    for g in np.flatnonzero(cls["real"]):
        want = level if level else (bc.LEVEL_IN if g % 2 == 0 else bc.LEVEL_OUT)
        assert abs(cls["amax"][g] - want) <= 1e-6 and (level or abs(cls["bmax"][g] - want) <= 1e-6), (g, cls["amax"][g], cls["bmax"][g])
    others = np.setdiff1d(np.arange(B), c["carriers"])
    assert fwd["a"][others].max() <= 0.71 and fwd["b"][others].max() <= 0.71         # (0.42 with the user factor)


@pytest.mark.parametrize("name", [n for n in sorted(bc.CASES) if bc.CASES[n]["layout"] == "partial"])
def test_partial_batches_hold_a_fast_and_an_exact_wave_at_each_threshold(name, record_property):
    c, fwd, _ = _views(name)
    cls, B, R = fwd["cls"], c["B"], c["R"]
    ylo = bc.Y_LO_PAIRS if R >= 2 else bc.Y_LO_SINGLE
    even, odd = _groups(cls)
    assert B % 256 != 0 and not cls["neutral"].any() and len(even) and len(odd)
    lab = cls["label"]
    e = c["expect"]
    for k, t in enumerate(e["in_tiles"]):
        assert (lab[even, t] == "fast").all() and (lab[odd, t] == "exact").all(), (t, lab[:, t])
        field, edge = (("xlo", bc.X_LO), ("yhi", bc.Y_HI), ("ylo", ylo))[k % 3]
        assert all(_near(cls[field][g, t], edge * 0.995) for g in even), (t, cls[field][:, t])
        assert all(_near(cls[field][g, t], edge * 0.995 * bc.LEVEL_OUT / bc.LEVEL_IN) for g in odd), (t, cls[field][:, t])
    for t in e["out_tiles"]:
        assert (lab[cls["real"], t] == "exact").all(), (t, lab[:, t])
    last = (B - 1) // 64
    assert last in e["out_tiles"] and B % 64 != 0 and _near(cls["yhi"][0, last], bc.Y_HI * 1.005)      # the partial tile's edge
    tame = np.setdiff1d(np.arange(lab.shape[1]), e["in_tiles"] + e["out_tiles"])
    assert (lab[:, tame] == "fast").all()
    if R >= 2:
        assert B % (64 * R) != 0                      # pad rows in the last row group: the (2h + 1) % R pairing meets them
    if R == 4 and B > 4096:
        assert (lab[cls["real"]] == "exact").sum() >= 1 and B - (B // 256) * 256 == 4
    record_property("labels", bc.label_counts(cls))
    print(name, bc.label_counts(cls))


@pytest.mark.parametrize("name", [n for n in sorted(bc.CASES) if bc.CASES[n]["layout"] == "full"])
def test_full_batches_hold_the_8_and_9_flag_tiles(name, record_property):
    c, fwd, _ = _views(name)
    cls, B = fwd["cls"], c["B"]
    e = c["expect"]
    even, odd = _groups(cls)
    real = np.flatnonzero(cls["real"])
    assert B % 256 == 0 and len(even) and len(odd)
    want = np.zeros(B // 64, int)
    for t, k in e["count"].items():
        want[t] = k
    assert np.array_equal(cls["count"], want), cls["count"]
    assert np.array_equal(np.flatnonzero(cls["flags"]), sorted(c["cols"]))             # exactly the edge columns are flagged
    small = (want > 0) & (want <= 8)
    lab = cls["label"]
    if c["neutral"]:
        assert np.array_equal(cls["neutral_tile"], small)
        assert np.array_equal(np.flatnonzero(cls["neutral"]), [k for k in sorted(c["cols"]) if small[k // 64]])
        assert (lab[:, small] == "fast").all()          # their flagged columns rotate as (0, 0)
    else:
        assert not cls["neutral"].any() and (lab[:, small][real] == "exact").all()
    t = e["flagged_fast_tile"]                        # 9 flags, none neutralised, all inside the wave's window at LEVEL_IN
    assert want[t] == 9 and (lab[even, t] == "fast").all() and (lab[odd, t] == "exact").all()
    assert all(_near(cls["xlo"][g, t], bc.X_LO * 0.995) and _near(cls["yhi"][g, t], bc.Y_HI * 0.995) for g in even)
    if c["R"] >= 2:
        assert all(_near(cls["ylo"][g, t], bc.Y_LO_PAIRS * 0.995) for g in even)
    if "nine_exact_tile" in e:                        # 9 flags, one of them outside the window at either level
        t = e["nine_exact_tile"]
        assert want[t] == 9 and (lab[real, t] == "exact").all() and all(_near(cls["xlo"][g, t], bc.X_LO * 1.005) for g in even)
    elif name not in ("rows2_full", "rows4_full", "neutral_off", "neutral_on"):
        raise AssertionError("a default-R full case needs the 9-flag exact tile")
    lane = np.array([k for k in c["cols"] if k // 64 == e["lane_tile"]])
    assert len(lane) == 8 and (lane % 64 < 16).all()                                  # one lane of the neutral block's scan
    spread = np.array([k for k in c["cols"] if k // 64 == e["spread_tile"]])
    assert len(spread) == 8 and np.array_equal(np.bincount(spread % 64 // 16, minlength=4), [2, 2, 2, 2])
    assert cls["flags"][0] and cls["flags"][63]
    if name == "full_r1":
        t = e["second_trip_tile"]
        assert t * 64 >= 1024 and want[t] == 8 and cls["neutral_tile"][t] and cls["flags"][64 * t] and cls["flags"][64 * t + 63]
        assert cls["neutral"][:1024].any()            # (the scan's column counter arrives there carried over)
    neu = cls["neutral"] if c["neutral"] else cls["flags"]
    p, n = fwd["p"], fwd["n"]
    assert (p[neu] < -20).any() and (n[neu] > 6).any() and (n[neu] < -60).any()        # flags of all three kinds
    record_property("labels", bc.label_counts(cls))
    print(name, bc.label_counts(cls))


def test_item_branch_rows_with_a_equal_to_one(record_property):
    c, fwd, _ = _views("item_branch_a1")
    cls, e = fwd["cls"], c["expect"]
    real = np.flatnonzero(cls["real"])
    assert c["kind"] == oracle.LOSS_RUBIBCE and (cls["amax"][real] == np.float32(1.0)).all()     # sig(20) == 1.0f: equality
    assert (fwd["a"][c["carriers"]] == np.float32(1.0)).all()
    want = np.zeros(c["B"] // 64, int)
    for t, k in e["count"].items():
        want[t] = k
    assert np.array_equal(cls["count"], want)
    t = e["a1_tile"]                                  # raw p = -19.9: unflagged, inside the window at amax = 1
    assert (cls["label"][real, t] == "fast").all() and all(_near(cls["xlo"][g, t], -19.9) for g in real)
    t = e["neutral_a1_tile"]
    assert cls["neutral_tile"][t] and cls["neutral"].sum() == 2 and (cls["label"][:, t] == "fast").all()
    assert np.allclose(fwd["p"][cls["neutral"]], -20.1, rtol=1e-4)
    t = e["nine_exact_tile"]
    assert not cls["neutral_tile"][t] and (cls["label"][real, t] == "exact").all()
    record_property("labels", bc.label_counts(cls))
    print("item_branch_a1", bc.label_counts(cls))


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_the_oracle_alone_leaves_room_and_every_edge_column_weighs(name, record_property):
    """|oracle - float64| <= a third of the GPU test's tolerances (losses 1e-5; gradients rtol 5e-4, atol 2e-6 max), and each
    edge or neutralised column holds at least 1e-4 of L_ori (float64): ten times the loss tolerance, so a column lost (or
    counted twice, which moves L_ori by the same amount) cannot pass."""
    c, fwd, ref = _views(name)
    third = 1e-5 / 3
    d_ori = abs(float(fwd["l_ori"]) - ref["l_ori"]) / ref["l_ori"]
    reg = oracle.l2_reg(c["P"][c["u"]], c["Q"][c["i"]], c["Q"][c["j"]], bc.DECAY, bc.BS)
    total = float(np.float32(fwd["mf"]) + np.float32(reg))
    d_tot = abs(total - ref["loss"]) / ref["loss"]
    record_property("oracle_vs_f64_l_ori", d_ori)
    record_property("oracle_vs_f64_loss", d_tot)
    print("%s: L_ori %.9g (float64 %.12g) rel %.3e; loss %.9g (%.12g) rel %.3e" % (name, fwd["l_ori"], ref["l_ori"], d_ori, total,
                                                                               ref["loss"], d_tot))
    assert d_ori <= third and d_tot <= third
    coef = bc.DECAY / bc.BS
    eu, ei, ej = c["P"][c["u"]], c["Q"][c["i"]], c["Q"][c["j"]]
    worst = {}
    for key, got, want in (("deu", fwd["deu"] + np.float32(coef) * eu, ref["deu"]), ("dei", fwd["dei"] + np.float32(coef) * ei, ref["dei"]),
                           ("dej", fwd["dej"] + np.float32(coef) * ej, ref["dej"]), ("dw", fwd["dw"], ref["dw"]), ("dwu", fwd["dwu"], ref["dwu"])):
        bound = (5e-4 * np.abs(want) + 2e-6 * np.abs(want).max()) / 3 + 1e-300
        worst[key] = float(np.max(np.abs(got - want) / bound))
        record_property("oracle_vs_f64_%s_over_bound" % key, worst[key])
    # dp, dn and the derivatives by si, sj (da, db times the sigmoid's slope, + the item term) of the oracle, read back out of
    # its rows dei = dp eu + dsi w, dej = dn eu + dsj w by least squares in float64
    w64 = c["w"].astype(np.float64)
    for key, rows, col, s_key in (("dp", fwd["dei"], "dp", "dsi"), ("dn", fwd["dej"], "dn", "dsj")):
        got = np.array([np.linalg.lstsq(np.stack([eu[k].astype(np.float64), w64], 1), rows[k].astype(np.float64), rcond=None)[0]
                        for k in range(c["B"])])
        for k2, (nm, want) in enumerate(((col, ref[col]), (s_key, ref[s_key]))):
            bound = (5e-4 * np.abs(want) + 2e-6 * np.abs(want).max()) / 3 + 1e-300
            worst[nm] = float(np.max(np.abs(got[:, k2] - want) / bound))
            record_property("oracle_vs_f64_%s_over_bound" % nm, worst[nm])
    print(name, "worst |oracle - float64| / (bound / 3):", worst)
    assert max(worst.values()) <= 1.0, worst
    watched = sorted(set(c["cols"]) | set(np.flatnonzero(fwd["cls"]["neutral"]).tolist()))
    share = ref["col_l"][watched] / ref["l_ori"]
    record_property("lightest_edge_column_share", float(share.min()))
    print(name, "lightest edge column: %.3e of L_ori (column %d)" % (share.min(), watched[int(share.argmin())]))
    assert share.min() >= 1e-4
    assert np.isfinite(fwd["deu"]).all() and np.isfinite(fwd["dei"]).all() and np.isfinite(fwd["dej"]).all()
