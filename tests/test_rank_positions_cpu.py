"""Full-catalogue positions without a GPU: the two entry points are declared, bound and exported; their refusals come before
any device work (the pointers below are never dereferenced, as in tests/test_sweep_args_cpu.py); the workspace size; and
macr_amd/rank_report.py against a brute-force restatement and the rank-sum AUC."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_ref
from helpers import REPO

U, N, D, NP = 300, 2500, 64, 1234


@pytest.fixture(scope="module")
def lib():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    """a 256-byte aligned host address standing in for every buffer"""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, base


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported(lib):
    L = lib.lib()
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(macr_[a-z0-9_]+)\s*\(", src))
    for name in ("macr_rank_positions_workspace_bytes", "macr_score_pairs", "macr_rank_positions"):
        assert name in declared and name in lib.SIGNATURES and hasattr(L, name), name
    assert sorted(lib.SIGNATURES) == sorted(declared)
    assert len(lib.SIGNATURES["macr_score_pairs"][1]) == 16 and len(lib.SIGNATURES["macr_rank_positions"][1]) == 20
    assert "item_offset" not in src[src.index("macr_rank_positions_workspace_bytes(int U"):]      # no item sharding yet
    # additive: the version the existing tests pin
    assert L.macr_abi_version() == 16 == lib.ABI_VERSION and re.search(r"#define MACR_ABI_VERSION\s+16\b", src)


def rank_call(lib, mem, **over):
    p = ctypes.c_void_p(mem[1])
    L = lib.lib()
    a = dict(kind=lib.SCORE_RUBI_BOTH, U=U, N=N, d=D, users=p, user_ids=p, items=p, sig_u=p, sig_i=p, c=0.5, c_dev=None,
             mask_ptr=p, mask_idx=p, pair_ptr=p, pair_item=p, n_pairs=NP, out=p, ws=p, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.macr_rank_positions_workspace_bytes(U, NP, N, D)
    return L.macr_rank_positions(a["kind"], a["U"], a["N"], a["d"], a["users"], a["user_ids"], a["items"], a["sig_u"], a["sig_i"],
                                 a["c"], a["c_dev"], a["mask_ptr"], a["mask_idx"], a["pair_ptr"], a["pair_item"], a["n_pairs"],
                                 a["out"], a["ws"], a["ws_bytes"], None)


def pairs_call(lib, mem, **over):
    p = ctypes.c_void_p(mem[1])
    a = dict(kind=lib.SCORE_RUBI_BOTH, U=U, N=N, d=D, users=p, user_ids=p, items=p, sig_u=p, sig_i=p, c=0.5, c_dev=None,
             pair_ptr=p, pair_item=p, n_pairs=NP, out=p)
    a.update(over)
    return lib.lib().macr_score_pairs(a["kind"], a["U"], a["N"], a["d"], a["users"], a["user_ids"], a["items"], a["sig_u"],
                                      a["sig_i"], a["c"], a["c_dev"], a["pair_ptr"], a["pair_item"], a["n_pairs"], a["out"], None)


def test_rank_positions_refuses_with_its_documented_codes(lib, mem):
    L = lib.lib()
    need = L.macr_rank_positions_workspace_bytes(U, NP, N, D)
    refused = [
        ("no kind at all", dict(kind=5), lib.E_INVALID, b"score_kind=5"),
        ("a negative kind", dict(kind=-1), lib.E_INVALID, b"score_kind=-1"),
        ("d = 48", dict(d=48), lib.E_UNSUPPORTED, b"d=48"),
        ("no queries", dict(U=0), lib.E_INVALID, b"U=0"),
        ("no items", dict(N=0), lib.E_INVALID, b"n_local=0"),
        ("a negative pair count", dict(n_pairs=-1), lib.E_INVALID, b"n_pairs=-1"),
        ("more pairs than an int32 CSR holds", dict(n_pairs=1 << 31), lib.E_INVALID, b"n_pairs=2147483648"),
        ("no user table", dict(users=None), lib.E_INVALID, b"null pointer"),
        ("no item table", dict(items=None), lib.E_INVALID, b"null pointer"),
        ("no pair CSR", dict(pair_ptr=None), lib.E_INVALID, b"null pointer"),
        ("no pair items", dict(pair_item=None), lib.E_INVALID, b"null pointer"),
        ("RUBI_BOTH without sig_u", dict(sig_u=None), lib.E_INVALID, b"sig_u"),
        ("DIRECT_MINUS_BOTH without sig_u", dict(kind=lib.SCORE_DIRECT_MINUS_BOTH, sig_u=None), lib.E_INVALID, b"sig_u"),
        ("RUBI without sig_i", dict(kind=lib.SCORE_RUBI, sig_i=None), lib.E_INVALID, b"sig_i"),
        ("DIRECT_MINUS without sig_i", dict(kind=lib.SCORE_DIRECT_MINUS, sig_i=None), lib.E_INVALID, b"sig_i"),
        ("half a mask", dict(mask_idx=None), lib.E_INVALID, b"mask_ptr and mask_idx"),
        ("no output", dict(out=None), lib.E_INVALID, b"out_pos"),
        ("no workspace", dict(ws=None), lib.E_INVALID, b"workspace"),
        ("an unaligned workspace", dict(ws=ctypes.c_void_p(mem[1] + 8)), lib.E_INVALID, b"workspace"),
        ("a workspace one byte short", dict(ws_bytes=need - 1), lib.E_WORKSPACE, b"workspace"),
        ("the workspace of fewer pairs", dict(ws_bytes=L.macr_rank_positions_workspace_bytes(U, NP // 2, N, D)), lib.E_WORKSPACE,
         b"workspace"),
    ]
    for name, over, code, text in refused:
        rc = rank_call(lib, mem, **over)
        assert rc == code, (name, rc, L.macr_last_error())
        msg = L.macr_last_error()
        assert b"rank_positions" in msg and text in msg, (name, msg)
    # kinds that read less pass the pointer checks without it: the call gets as far as the workspace check
    for over in (dict(kind=lib.SCORE_NORMAL, sig_i=None, sig_u=None), dict(kind=lib.SCORE_RUBI, sig_u=None),
                 dict(kind=lib.SCORE_DIRECT_MINUS, sig_u=None), dict(mask_ptr=None, mask_idx=None, user_ids=None)):
        assert rank_call(lib, mem, ws_bytes=16, **over) == lib.E_WORKSPACE, (over, L.macr_last_error())
    # nothing to rank: no device work, no output needed
    assert rank_call(lib, mem, n_pairs=0, out=None, pair_item=None) == lib.OK


def test_score_pairs_refuses_with_its_documented_codes(lib, mem):
    L = lib.lib()
    refused = [
        ("no kind at all", dict(kind=5), lib.E_INVALID, b"score_kind=5"),
        ("d = 48", dict(d=48), lib.E_UNSUPPORTED, b"d=48"),
        ("no queries", dict(U=-3), lib.E_INVALID, b"U=-3"),
        ("a negative pair count", dict(n_pairs=-7), lib.E_INVALID, b"n_pairs=-7"),
        ("no item table", dict(items=None), lib.E_INVALID, b"null pointer"),
        ("no pair CSR", dict(pair_ptr=None), lib.E_INVALID, b"null pointer"),
        ("RUBI_BOTH without sig_u", dict(sig_u=None), lib.E_INVALID, b"sig_u"),
        ("RUBI without sig_i", dict(kind=lib.SCORE_RUBI, sig_i=None), lib.E_INVALID, b"sig_i"),
        ("no output", dict(out=None), lib.E_INVALID, b"out_scores"),
    ]
    for name, over, code, text in refused:
        rc = pairs_call(lib, mem, **over)
        assert rc == code, (name, rc, L.macr_last_error())
        msg = L.macr_last_error()
        assert b"score_pairs" in msg and text in msg, (name, msg)
    assert pairs_call(lib, mem, n_pairs=0, out=None, pair_item=None) == lib.OK


def test_workspace_size(lib):
    ws = lib.lib().macr_rank_positions_workspace_bytes
    for bad in [(U, NP, N, 48), (U, NP, N, 0), (0, NP, N, D), (-1, NP, N, D), (U, -1, N, D), (U, NP, 0, D), (U, NP, -5, D),
                (U, 1 << 31, N, D)]:
        assert ws(*bad) == 0, bad
    for u, n, d in [(U, N, D), (1, 5, 32), (37, 333, 128), (15424, 40981, 256)]:
        sizes = [ws(u, p, n, d) for p in (0, 1, 15, 16, 17, 1000, 1001, 123456, (1 << 31) - 1)]
        assert sizes[0] > 0 and all(s % 16 == 0 for s in sizes), sizes
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes            # monotone in n_pairs
        assert sizes[5] >= 1000 * 12                                             # a key and a counter per pair, at least
        assert ws(u, 1000, n, d) == ws(u, 1000, n + 7, d)                        # the catalogue never enters the workspace


# ----------------------------------------------------------------------------- rank_report.summarize
def brute_force(scores, mask_lists, gt_lists, group_of=None, n_groups=0):
    """every user's candidates sorted by (-score, id); (negative, positive) pairs counted one by one"""
    aucs, rrs, pcts, users, skipped = [], [], [], 0, 0
    g_cnt, g_sum = np.zeros(n_groups, dtype=np.int64), np.zeros(n_groups, dtype=np.float64)
    for q in range(scores.shape[0]):
        masked = set(mask_lists[q])
        cand = [i for i in range(scores.shape[1]) if i not in masked]
        pos_items = [g for g in gt_lists[q] if g not in masked and 0 <= g < scores.shape[1]]
        skipped += len(gt_lists[q]) - len(pos_items)
        order = sorted(cand, key=lambda i: (-float(scores[q, i]), i))
        is_pos = [i in set(pos_items) for i in order]
        m, nn = len(pos_items), len(cand) - len(pos_items)
        if m == 0 or nn == 0:
            skipped += m
            continue
        users += 1
        wins, neg_above, first = 0, 0, None
        for idx, (item, p) in enumerate(zip(order, is_pos)):
            if not p:
                neg_above += 1
                continue
            first = idx if first is None else first
            for later in is_pos[idx + 1:]:              # the negatives this positive beats, one by one
                wins += 0 if later else 1
            pcts.append(neg_above / nn)
            if group_of is not None:
                g_cnt[group_of[item]] += 1
                g_sum[group_of[item]] += neg_above / nn
        aucs.append(wins / (m * nn))
        rrs.append(1.0 / (first + 1))
    return dict(users=users, pairs=len(pcts), skipped=skipped, auc=np.mean(aucs), mrr=np.mean(rrs), mpr=np.mean(pcts),
                group_pairs=g_cnt, group_sum=g_sum)


def csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    idx = np.asarray([x for r in lists for x in sorted(r)], dtype=np.int64)
    return ptr, idx


def population(rs, n_users, n_items, ties):
    scores = rs.standard_normal((n_users, n_items)).astype(np.float32)
    if ties:
        scores = (np.round(scores * 2.0) / 2.0).astype(np.float32)
    mask = [sorted(rs.choice(n_items, rs.randint(0, n_items // 2), replace=False).tolist()) for _ in range(n_users)]
    gt = [sorted(rs.choice(n_items, rs.randint(0, 9), replace=False).tolist()) for _ in range(n_users)]
    mask[1] = sorted(set(range(n_items)) - set(gt[1][:1]))[:n_items - 1]         # one candidate left
    gt[2] = sorted(set(range(n_items)) - set(mask[2]))                          # m = n_cand: no negatives
    gt[3] = []
    if gt[4]:
        mask[4] = sorted(set(mask[4]) | {gt[4][0]})                              # a held-out item that is also a train item
    return scores, mask, gt


@pytest.mark.parametrize("ties", [False, True])
def test_summarize_equals_the_brute_force(ties):
    from macr_amd import rank_report
    rs = np.random.RandomState(11 + ties)
    n_users, n_items = 40, 57
    scores, mask, gt = population(rs, n_users, n_items, ties)
    group_of = rs.randint(0, 6, n_items)
    pos = rank_ref.positions(scores, mask, gt)
    ptr, idx = csr(gt)
    n_cand = np.asarray([n_items - len(m) for m in mask])
    got = rank_report.summarize(pos, ptr, idx, n_cand, group_of, 6)
    want = brute_force(scores, mask, gt, group_of, 6)
    assert (got["users"], got["pairs"], got["skipped"]) == (want["users"], want["pairs"], want["skipped"])
    assert got["users"] > 20 and got["skipped"] > 0 and got["pairs"] + got["skipped"] == len(pos)
    for k in ("auc", "mrr", "mpr"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=k)
    assert np.array_equal(got["group_pairs"], want["group_pairs"]) and got["group_pairs"].sum() == got["pairs"]
    full = want["group_pairs"] > 0
    np.testing.assert_allclose(got["group_mpr"][full], want["group_sum"][full] / want["group_pairs"][full], rtol=1e-12)
    assert np.all(np.isnan(got["group_mpr"][~full]))
    # without groups: the same numbers, no group keys
    plain = rank_report.summarize(pos, ptr, idx, n_cand)
    assert "group_pairs" not in plain and plain["auc"] == got["auc"] and plain["mpr"] == got["mpr"]
    if ties:
        return
    # no ties: the AUC is the rank-sum (Mann-Whitney) statistic of the scores, computed on its own
    aucs = []
    for q in range(n_users):
        cand = np.setdiff1d(np.arange(n_items), mask[q])
        p = np.intersect1d(gt[q], cand)
        if len(p) == 0 or len(p) == len(cand):
            continue
        s = scores[q, cand].astype(np.float64)
        assert len(np.unique(s)) == len(s)
        ranks = np.empty(len(s)); ranks[np.argsort(s)] = np.arange(1, len(s) + 1)      # ascending ranks, 1-based
        r_pos = ranks[np.isin(cand, p)].sum()
        aucs.append((r_pos - len(p) * (len(p) + 1) / 2) / (len(p) * (len(cand) - len(p))))
    np.testing.assert_allclose(got["auc"], np.mean(aucs), rtol=1e-12)


def test_summarize_hand_cases():
    from macr_amd.rank_report import summarize, format_line
    one = lambda pos, ptr, n_cand, **kw: summarize(pos, ptr, np.arange(len(pos)), n_cand, **kw)
    # one pair at position 0 of 10 candidates: above all 9 negatives
    r = one([0], [0, 1], [10])
    assert (r["users"], r["pairs"], r["skipped"], r["auc"], r["mrr"], r["mpr"]) == (1, 1, 0, 1.0, 1.0, 0.0)
    # all pairs last: 3 positives at the bottom of 10 candidates
    r = one([7, 8, 9], [0, 3], [10])
    assert (r["auc"], r["mpr"], r["pairs"]) == (0.0, 1.0, 3) and r["mrr"] == 1.0 / 8
    # positions in CSR order need not ascend: item order is by id, not by rank
    r = one([9, 0, 4], [0, 3], [10])
    np.testing.assert_allclose([r["auc"], r["mrr"], r["mpr"]], [1 - (0 + 3 / 7 + 1) / 3, 1.0, (0 + 3 / 7 + 1) / 3], rtol=1e-15)
    # m = n_cand: no negative to be above of -> skipped; a query without pairs; a -1 pair beside a valid one
    r = one([0, 1, 2, 5, -1], [0, 3, 3, 5], [3, 8, 12])
    assert (r["users"], r["pairs"], r["skipped"]) == (1, 1, 4)
    np.testing.assert_allclose([r["auc"], r["mrr"], r["mpr"]], [1 - 5 / 11, 1 / 6, 5 / 11], rtol=1e-15)
    # nothing to count at all: nan, not an exception
    r = one([-1, -1], [0, 2], [5], group_of=[0, 1], n_groups=2)
    assert (r["users"], r["pairs"], r["skipped"]) == (0, 0, 2) and np.isnan(r["auc"]) and np.isnan(r["mrr"]) and np.isnan(r["mpr"])
    assert r["group_pairs"].tolist() == [0, 0] and np.all(np.isnan(r["group_mpr"]))
    with pytest.raises(ValueError):
        one([0, 1], [0, 1], [10])
    # the line of the command lines
    r = summarize([0, 3], [0, 1, 2], [4, 2], [10, 5], group_of=[0, 0, 5, 0, 1], n_groups=6)
    assert format_line(r) == ("rank: users=2 pairs=2 skipped=0 auc=0.62500 mrr=0.62500 mpr=0.37500 | train-popularity groups "
                              "(<10,<50,<100,<200,<500,>=500): pairs=[0, 1, 0, 0, 0, 1] mpr=[nan, 0.00000, nan, nan, nan, 0.75000]")


def test_rank_report_switch_is_the_environment(monkeypatch):
    from macr_amd import rank_report
    monkeypatch.delenv("MACR_RANK_REPORT", raising=False)
    assert not rank_report.enabled()
    monkeypatch.setenv("MACR_RANK_REPORT", "0")
    assert not rank_report.enabled()
    monkeypatch.setenv("MACR_RANK_REPORT", "1")
    assert rank_report.enabled()
    # the parsers keep their flag sets: the switch is no flag
    for path in ("macr_mf/parse.py", "macr_lightgcn/utility/parser.py"):
        assert "rank_report" not in open(os.path.join(REPO, path)).read().lower()
