"""The cases of tests/seg_cases.py really contain what they exist for (no GPU): every prescribed run lies where its case says --
window offset, block straddle, number of following windows, end of the list -- the int64 sums are exact in fp32 in any order,
every case fits the slots of the deterministic workspace and the work list of INDEX mode, and the sort's workspace rule
(refsort.hpp::sort_hist_words) covers every smaller sort at the tile that sort takes, with and without MACR_SORT_TILE.
tests/test_gpu_seg_exact.py and tests/test_gpu_refsort.py rest on this."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import refsort_worker as rw
import seg_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=sc.DIMS)
def d(request):
    return request.param


def _find(c, table, start):
    for rec in sc.layout(c):
        if rec["table"] == table and rec["start"] == start:
            return rec
    raise AssertionError("%s d=%d: no run of table %s begins at %d" % (c["name"], c["d"], table, start))


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_every_prescribed_run_lies_where_its_case_says(d, name):
    c = sc.case(d, name)
    CH, R, n, B = sc.ch_of(d), sc.rpb_of(d), c["n"], c["B"]
    lay = sc.layout(c)
    sk, sv = sc.sorted_list(c)
    n_ul, n_il = c["owned"][2], c["owned"][5]
    # the list the builder laid out is the list the keys sort to: the same runs at the same positions
    assert [(r["table"], r["start"], r["len"]) for r in lay] == c["runs"]
    assert len(c["u"]) == len(c["i"]) == len(c["j"]) == B and c["stage"].shape == (n, d)
    for arr, rows in ((c["u"], c["n_users"]), (c["i"], c["n_items"]), (c["j"], c["n_items"])):
        assert arr.min() >= 0 and arr.max() < rows
    if not c["sharded"]:
        assert c["owned"] == (0, 1, c["n_users"], 0, 1, c["n_items"]) and int((sk < n_ul + n_il).sum()) == n
        # the batch is no sorted list: a sort that did nothing would show
        assert not np.array_equal(sv, np.arange(n)) or name == "index_one_row"
    for table, start, L, tag in c["want"]:
        rec = _find(c, table, start)
        assert rec["len"] == L == tag.get("len", L), (name, tag, rec)
        assert rec["nc"] == (start + L - 1) // CH - start // CH and rec["inv_nc"] == (L - 1) // CH
        assert rec["multi"] == (L > CH - start % CH) and rec["inv_multi"] == (L > CH)
        if "off" in tag:
            assert rec["off"] == tag["off"], (name, tag, rec)
        if "straddle" in tag:
            assert rec["straddle"] and start // R != (start + L - 1) // R
        if "nc" in tag:
            assert rec["nc"] == tag["nc"]
        if "min_nc" in tag:
            assert rec["nc"] >= tag["min_nc"] and rec["inv_nc"] >= tag["min_nc"] and len(rec["work"]) >= 100
        if "ends_on_window" in tag:
            assert ((start + L) % CH == 0) == tag["ends_on_window"] and start + L < n
        if tag.get("last"):
            assert rec["last"] and start + L == n and rec["table"] == "i"
        if tag.get("fold_hits_nwin"):
            assert rec["fold_hits_nwin"] and rec["inv_hits_n"] == (L > CH)       # (k_seg_fold_inv: only a run longer than CH has an owner)
        if "start" in tag:
            assert start == tag["start"]
        if tag.get("last_owned"):
            nxt = start + L
            if table == "i" or n_il == 0:
                assert nxt == int((sk < n_ul + n_il).sum()) and nxt < n and sk[nxt] == n_ul + n_il     # foreign keys follow at once
    # rows: row 0 and the last row of each table are referenced, and some row in between is not
    for table, nl in (("u", n_ul), ("i", n_il)):
        rows = sorted(r["row"] for r in lay if r["table"] == table)
        if rows:
            assert rows[0] == 0 and rows[-1] == nl - 1
        if len(rows) > 4:
            assert len(rows) < nl


def _by_len(c):
    out = {}
    for rec in sc.layout(c):
        out.setdefault(rec["len"], []).append(rec)
    return out


def test_run_lengths_at_their_offsets_and_across_block_edges(d):
    CH, R = sc.ch_of(d), sc.rpb_of(d)
    assert sorted(set([1, CH - 1, CH, CH + 1, 16, 17, 2 * CH, 2 * CH + 1, 63, 64, 65, 128, 129])) == sorted(sc.lens_of(d))
    for name, off in (("lengths_off0", 0), ("lengths_off1", 1), ("lengths_offlast", CH - 1)):
        by = _by_len(sc.case(d, name))
        for L in sc.lens_of(d):
            if L == 1:
                continue                                # (the filler rows are runs of 1 at every offset)
            assert [r["off"] for r in by[L]] == [off, off], (name, L)          # once per table
            assert sorted(r["table"] for r in by[L]) == ["i", "u"]
    by = _by_len(sc.case(d, "lengths_straddle"))
    for L in sc.lens_of(d):
        if L == 1:
            continue
        recs = [r for r in by[L] if r["straddle"]]
        assert len(recs) >= 4
        # the edge directly behind the first reference, and directly before the last
        assert any((r["start"] + 1) % R == 0 for r in recs) and any((r["start"] + L - 1) % R == 0 for r in recs)
    # both kinds of head in one block, a head whose chunk is cut by the window and one cut by the run's end
    c = sc.case(d, "lengths_offlast")
    assert any(r["multi"] and len(r["heads"]) >= 3 and r["heads"][1] - r["heads"][0] == 1 for r in sc.layout(c))


def test_fold_chunk_counts_cover_every_tail_branch(d):
    """k_seg_fold / k_seg_fold_inv: nc = 1 .. 9 and >= 1000, each ending inside the list off a window edge, on a window edge, and
    as the last run of the list (hi == nwin; k_seg_scan's gallop past n)"""
    CH = sc.ch_of(d)
    inside = {r["nc"]: r for r in sc.layout(sc.case(d, "nc_inside")) if r["off"] == 3 and r["len"] > 2}
    edge = {r["nc"]: r for r in sc.layout(sc.case(d, "nc_window_edge")) if r["off"] == 3 and r["len"] > 2}
    assert sorted(inside) == sorted(edge) == list(range(1, 10))
    assert all((r["start"] + r["len"]) % CH == 2 and not r["fold_hits_nwin"] for r in inside.values())
    assert all((r["start"] + r["len"]) % CH == 0 and not r["last"] for r in edge.values())
    assert sorted(set(r["inv_nc"] for r in edge.values())) == list(range(1, 10))
    last_full = []
    for k in range(1, 10):
        c = sc.case(d, "nc_last_%d" % k)
        rec = sc.layout(c)[-1]
        assert rec["last"] and rec["nc"] == k and rec["fold_hits_nwin"] and rec["inv_hits_n"] == (rec["len"] > CH) and rec["off"] == 3
        assert rec["len"] <= sc.K_REF_RUN or rec["scan_past_n"]          # k_seg_scan's gallop leaves the list: lo + step > n
        last_full.append(c["n"] % CH == 0)
    assert any(last_full) and not all(last_full)             # the last window full, and partial
    assert any(sc.layout(sc.case(d, "nc_last_%d" % k))[-1]["scan_past_n"] for k in range(1, 10))
    for name, on_edge, last in (("nc_big_inside", False, False), ("nc_big_window_edge", True, False), ("nc_big_last", False, True)):
        c = sc.case(d, name)
        rec = max(sc.layout(c), key=lambda r: r["len"])
        assert rec["nc"] >= 1000 and rec["inv_nc"] >= 1000 and rec["last"] == last and (rec["fold_hits_nwin"] or not last)
        if not last:
            assert ((rec["start"] + rec["len"]) % CH == 0) == on_edge
        assert c["stage"].nbytes <= 32 << 20
    # a single reference ends the list too (lim = n - p = 1 in k_seg_scan), and a run of <= 16 cut short by the end of the list
    assert sc.layout(sc.case(d, "list_edges"))[-1]["len"] == 1 and sc.layout(sc.case(d, "list_edges"))[-1]["scan_lim_cut"]
    assert any(sc.layout(sc.case(d, "nc_last_%d" % k))[-1]["scan_lim_cut"] for k in range(1, 10))


def test_list_edges(d):
    CH, R = sc.ch_of(d), sc.rpb_of(d)
    c = sc.case(d, "list_edges")
    lay = sc.layout(c)
    assert c["n"] % CH != 0 and c["n"] % R != 0
    assert lay[0]["start"] == 0 and lay[0]["len"] == 129 and lay[0]["table"] == "u"
    last_u = [r for r in lay if r["table"] == "u"][-1]
    first_i = [r for r in lay if r["table"] == "i"][0]
    assert last_u["len"] == 65 and first_i["len"] == 65 and last_u["start"] + 65 == first_i["start"] == c["B"]
    assert last_u["row"] == c["owned"][2] - 1 and first_i["row"] == 0        # the is_user switch between two long runs
    # (some case with n a multiple of CH, too)
    assert any(sc.case(d, n)["n"] % CH == 0 for n in sc.CASE_NAMES)


def test_index_mode_capacity(d):
    """the work list lives in the sort's free key buffer, 3B words, two per item"""
    for name in sc.CASE_NAMES:
        c = sc.case(d, name)
        items = sum(len(r["work"]) for r in sc.layout(c))
        assert 2 * items <= c["n"], (name, items)
        for r in sc.layout(c):
            assert (r["flag"] == 1) == (r["len"] > sc.K_REF_RUN)
            if r["flag"] != 1:
                assert r["flag"] >> sc.K_REF_SHIFT == r["len"] and r["flag"] & ((1 << sc.K_REF_SHIFT) - 1) == r["start"]
            else:
                assert sum(s for _, s in r["work"]) == r["len"] and r["work"][0][0] == r["start"]
                assert all(s == sc.K_LONG_SPAN for _, s in r["work"][:-1])
    c = sc.case(d, "index_all_17")
    lay = sc.layout(c)
    assert all(r["len"] == 17 and len(r["work"]) == 1 for r in lay) and 17 * len(lay) == c["n"]
    c = sc.case(d, "index_one_row")
    lay = sc.layout(c)
    assert len(lay) == 2 and sum(r["len"] for r in lay) == c["n"] and all(r["flag"] == 1 for r in lay)


def test_ownership_cases(d):
    for name, (ust, ist) in (("own_interleaved", (3, 3)), ("own_range", (1, 1)), ("own_range_first", (1, 1))):
        c = sc.case(d, name)
        u_lo, u_st, n_ul, i_lo, i_st, n_il = c["owned"]
        assert c["sharded"] and (u_st, i_st) == (ust, ist) and (u_lo, u_st, i_lo, i_st) != (0, 1, 0, 1)
        keys = sc.ref_keys(c)
        foreign = keys == n_ul + n_il
        assert foreign[:c["B"]].sum() >= 5 and foreign[c["B"]:].sum() >= 5
        lay = sc.layout(c)
        assert lay[-1]["len"] >= 64 and lay[-1]["row"] == n_il - 1        # a long owned run, then the foreign keys
        # foreign rows on both sides of the owned ones, and (interleaved) between them
        fu = set(c["u"][foreign[:c["B"]]].tolist())
        assert u_lo + n_ul * u_st in fu and (u_lo == 0 or u_lo - 1 in fu) and (u_st == 1 or u_lo + 1 in fu)
    c = sc.case(d, "own_no_users")
    assert c["owned"][2] == 0 and all(r["table"] == "i" for r in sc.layout(c)) and sc.initial(c, "det")[0] is None
    c = sc.case(d, "own_nothing")
    assert sc.layout(c) == [] and c["owned"][2] > 0 and c["owned"][5] > 0
    assert np.all(sc.ref_keys(c) == c["owned"][2] + c["owned"][5])


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_sums_are_exact_and_the_slots_fit(d, name):
    c = sc.case(d, name)
    CH = sc.ch_of(d)
    SU, SI, cu, ci, bound = sc.row_sums(c)
    assert bound < 1 << 24, (name, bound)
    assert np.abs(c["stage"]).max() <= sc.STAGE_MAX and np.array_equal(c["stage"], np.round(c["stage"]))
    # a distinct pattern per reference and per column: no two staging rows of a run agree, no two columns either
    assert len(np.unique(c["stage"][:min(c["n"], 2000)], axis=0)) == min(c["n"], 2000)
    assert len(np.unique(c["stage"][:2000].T, axis=0)) == d
    nslots = 2 * ((c["n"] + CH - 1) // CH)                      # rows of cpart in the deterministic workspace
    for key in ("det_slots", "inv_slots"):
        slots = [s for r in sc.layout(c) for s in r[key]]
        assert len(slots) == len(set(slots)) and (not slots or max(slots) < nslots), (name, key)
    lay = sc.layout(c)
    assert int(cu.sum() + ci.sum()) == sum(r["len"] for r in lay)
    for mode in sc.MODES:
        ini, exp = sc.initial(c, mode), sc.expected(c, mode)
        for a, b in zip(ini, exp):
            assert (a is None) == (b is None)
            if a is not None:                           # the guard rows stay as they were
                assert np.array_equal(a[-sc.GUARD_ROWS:], b[-sc.GUARD_ROWS:])


def test_a_lost_reference_cannot_pass():
    assert sc.sensitivity_check() >= 6700                       # (the hot row of test_mf_large_batch_staged_path_matches_oracle)


@pytest.fixture(scope="module")
def ops():
    from macr_amd.build import build
    build()
    from macr_amd import ops as _ops
    return _ops


def test_sort_workspace_rule(ops):
    """sort_hist_words(n) over a sweep that crosses 2^17 and 2^20 (both +-1): non-decreasing, and >= 256 * ceil(m / tile) + 4 * 256
    for every m <= n of the sweep at the tile sort_tile_for(m) picks"""
    assert not os.environ.get("MACR_SORT_TILE")
    sweep = rw.hist_sweep()
    for e in (1 << 17, 1 << 20):
        assert {e - 1, e, e + 1} <= set(sweep)
    assert [ops.test_sort_tile_for(n) for n in (1 << 17, (1 << 17) + 1, 1 << 20, (1 << 20) + 1)] == [2048, 8192, 8192, 16384]
    assert rw.check_hist_rule(ops) == len(sweep)
    # the rule is tight where it matters: the step from 64 small tiles to 17 mid ones does not shrink the workspace
    assert ops.test_sort_hist_words((1 << 17) + 1) >= 256 * 64 + 1024


def test_sort_workspace_rule_under_a_forced_tile():
    """the same in a child process with MACR_SORT_TILE=2048 (the value is latched in a static)"""
    env = dict(os.environ, MACR_SORT_TILE="2048")
    r = subprocess.run([sys.executable, os.path.join(HERE, "refsort_worker.py"), "hist"], env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ok"] and verdict["tile"] == 2048 and verdict["done"] == len(rw.hist_sweep()), verdict
