"""The reference of tests/test_gpu_nonfinite.py held to its own rule, without a GPU: nonfinite_cases.expected() is the plain oracle
on finite tables, equals a numpy restatement of the rule on every case, every case has the property it is named for, and none is
vacuous (most queries keep a full list, few scores are NaN)."""
import numpy as np
import pytest

import nonfinite_cases as nf
import oracle

ALL = [(name, k) for name in nf.NAMES for k in range(len(nf.EPILOGUE_KINDS) * len(nf.EPILOGUE_CS) if name == "epilogue" else 1)]
_memo = {}


def solved(name, k=0, K=nf.K):
    """(case, score matrix, (val, idx, cnt) of expected()) -- computed once per case"""
    key = (name, k, K)
    if key not in _memo:
        case = nf.make(name)[k]
        su, si = nf.with_sigs(case)
        S = oracle.score_matrix(case.kind, case.P, case.Q, su, si, case.c)
        _memo[key] = (case, S, nf.expected_case(case, K))
    return _memo[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind,c", [(oracle.SCORE_NORMAL, 0.0), (oracle.SCORE_RUBI_BOTH, 40.0), (oracle.SCORE_DIRECT_MINUS_BOTH, -2.5)])
def test_on_finite_tables_expected_is_the_plain_oracle(kind, c):
    P, Q, sig_u, sig_i, mask = nf.base()
    su, si = (None, None) if kind == oracle.SCORE_NORMAL else (sig_u, sig_i)
    wv, wi, wc = oracle.score_topk(kind, P, Q, nf.K, su, si, c, oracle.csr_from_lists(mask))
    ev, ei, ec = nf.expected(kind, P, Q, nf.K, su, si, c, mask)
    assert np.array_equal(ei, wi) and np.array_equal(ec, wc) and np.array_equal(bits(ev), bits(wv))


@pytest.mark.parametrize("name,k", ALL)
def test_expected_is_the_restated_rule(name, k):
    case, S, (ev, ei, ec) = solved(name, k)
    rv, ri, rc = nf.restated(S, nf.K, case.mask)
    assert np.array_equal(ei, ri)
    assert np.array_equal(ec, rc)
    assert np.array_equal(bits(ev), bits(rv))
    assert not np.isnan(ev).any()
    # a short list is padded with (-inf, -1) and nothing else
    pad = np.arange(nf.K)[None, :] >= ec[:, None]
    assert (ei[pad] == -1).all() and (ei[~pad] >= 0).all() and np.isneginf(ev[pad]).all()


@pytest.mark.parametrize("K", [1, 32, 50, 128])
@pytest.mark.parametrize("name", ["nan_item", "overflow_many", "all_nan"])
def test_expected_is_the_restated_rule_at_the_other_Ks(name, K):
    case, S, (ev, ei, ec) = solved(name, 0, K)
    rv, ri, rc = nf.restated(S, K, case.mask)
    assert np.array_equal(ei, ri) and np.array_equal(ec, rc) and np.array_equal(bits(ev), bits(rv))


def test_expected_with_an_item_offset_is_the_shard_of_the_restated_rule():
    case = nf.make("overflow_many")[0]
    lo, hi = 1333, 2666
    ev, ei, ec = nf.expected(case.kind, case.P, case.Q[lo:hi], nf.K, None, None, 0.0, case.mask, item_offset=lo)
    S = oracle.score_matrix(case.kind, case.P, case.Q[lo:hi])
    rv, ri, rc = nf.restated(S, nf.K, case.mask, item_offset=lo)
    assert np.array_equal(ei, ri) and np.array_equal(ec, rc) and np.array_equal(bits(ev), bits(rv))
    assert ((ei >= lo) & (ei < hi) | (ei == -1)).all()


@pytest.mark.parametrize("name,k", [nk for nk in ALL if nk[0] != "all_nan"])
def test_no_case_is_vacuous(name, k):
    """at least 90 % of the queries keep a full list of K and under 5 % of the score matrix is NaN (all_nan excepted: it is
    about the opposite)"""
    case, S, (_, _, ec) = solved(name, k)
    assert (ec == nf.K).mean() >= 0.9
    assert np.isnan(S).mean() < 0.05
    assert not np.isfinite(S).all()                          # something non-finite does reach the ranking


def heavy_counts_stand(ec, but=()):
    for q in nf.HEAVY:
        if q not in but:
            assert ec[q] == nf.LEFT


def test_nan_query_has_count_0_and_nobody_else_changes():
    case, S, (ev, ei, ec) = solved("nan_query")
    P, Q, _, _, mask = nf.base()
    bv, bi, bc = oracle.score_topk(case.kind, P, Q, nf.K, mask=oracle.csr_from_lists(mask))
    assert np.isnan(S[nf.QA]).all() and np.isnan(S).sum() == nf.N
    assert ec[nf.QA] == 0 and (ei[nf.QA] == -1).all() and np.isneginf(ev[nf.QA]).all()
    others = np.arange(nf.U) != nf.QA
    assert np.array_equal(ei[others], bi[others]) and np.array_equal(bits(ev[others]), bits(bv[others]))
    assert np.array_equal(ec[others], bc[others])
    heavy_counts_stand(ec)


def test_nan_item_is_a_candidate_for_nobody():
    case, S, (ev, ei, ec) = solved("nan_item")
    assert np.isnan(S[:, nf.NAN_ITEM]).all() and np.isnan(S).sum() == nf.U
    assert not (ei == nf.NAN_ITEM).any()
    heavy_counts_stand(ec)
    # the plain oracle does list it while a list is short: the rule is not the oracle's own
    _, pi, _ = oracle.score_topk(case.kind, case.P, case.Q, nf.K, mask=oracle.csr_from_lists(case.mask))
    assert (pi == nf.NAN_ITEM).any()


def test_inf_query_scores_nan_on_the_zeros_and_inf_by_sign_elsewhere():
    case, S, (ev, ei, ec) = solved("inf_query")
    row = S[nf.QA]
    assert np.isnan(row[list(nf.ZERO_ITEMS)]).all() and np.isnan(S).sum() == len(nf.ZERO_ITEMS)
    rest = np.setdiff1d(np.arange(nf.N), nf.ZERO_ITEMS)
    assert np.array_equal(row[rest], np.where(case.Q[rest, nf.COL] > 0, np.inf, -np.inf).astype(np.float32))
    assert ec[nf.QA] == nf.K and np.isposinf(ev[nf.QA]).all()
    assert (np.diff(ei[nf.QA]) > 0).all()                    # ties at +inf: ascending id
    assert not np.isin(ei[nf.QA], nf.ZERO_ITEMS).any()


def test_inf_item_gives_both_infinities_and_no_nan():
    case, S, (ev, ei, ec) = solved("inf_item")
    assert not np.isnan(S).any()
    for it in (nf.INF_ITEM_POS, nf.INF_ITEM_NEG):
        assert np.isposinf(S[:, it]).sum() > 50 and np.isneginf(S[:, it]).sum() > 50
    free = np.array([nf.INF_ITEM_POS not in set(m) for m in case.mask])
    top = np.isposinf(S[:, nf.INF_ITEM_POS]) & free & ~np.isposinf(S[:, nf.INF_ITEM_NEG])
    assert top.sum() > 20 and (ei[top, 0] == nf.INF_ITEM_POS).all() and np.isposinf(ev[top, 0]).all()
    both = np.isposinf(S[:, nf.INF_ITEM_POS]) & np.isposinf(S[:, nf.INF_ITEM_NEG])
    both &= free & np.array([nf.INF_ITEM_NEG not in set(m) for m in case.mask])
    assert both.sum() > 20 and (ei[both, :2] == [nf.INF_ITEM_POS, nf.INF_ITEM_NEG]).all()      # a tie at +inf: the lower id first


def test_inf_minus_inf_is_nan_where_the_two_elements_share_a_sign():
    case, S, (ev, ei, ec) = solved("inf_minus_inf")
    P = case.P
    same = (P[:, 5] > 0) == (P[:, nf.COL2] > 0)
    assert np.array_equal(np.isnan(S[:, nf.NAN_ITEM]), same) and 50 < same.sum() < nf.U - 50
    assert np.isnan(S).sum() == same.sum()
    assert not (ei[same] == nf.NAN_ITEM).any()
    free = np.array([nf.NAN_ITEM not in set(m) for m in case.mask])
    first = ~same & (P[:, 5] > 0) & free
    assert first.sum() > 20 and (ei[first, 0] == nf.NAN_ITEM).all() and np.isposinf(ev[first, 0]).all()


@pytest.mark.parametrize("name,n_pos", [("overflow_many", 30), ("overflow_few", 3)])
def test_overflow_cases_tie_at_inf_from_finite_operands(name, n_pos):
    case, S, (ev, ei, ec) = solved(name)
    assert np.isfinite(case.P).all() and np.isfinite(case.Q).all()
    assert not np.isnan(S).any()
    pos, neg = nf.overflow_rows(n_pos)
    for q, hi_rows, lo_rows in ((nf.QA, pos, neg), (nf.QB, neg, pos)):
        assert np.isposinf(S[q, hi_rows]).all() and np.isneginf(S[q, lo_rows]).all()
        assert np.isinf(S[q]).sum() == n_pos + 5
        want = [i for i in hi_rows if i not in set(case.mask[q])][:nf.K]
        assert len(want) >= min(len(hi_rows), 3)
        assert ei[q, :len(want)].tolist() == want and np.isposinf(ev[q, :len(want)]).all()
        assert ec[q] == nf.K
        if len(want) < nf.K:
            assert np.isfinite(ev[q, len(want):]).all() and (np.diff(ev[q, len(want):]) <= 0).all()
    if name == "overflow_many":
        assert np.isposinf(ev[nf.QA]).sum() >= nf.K          # more than K ties at +inf
    assert np.isfinite(S[np.setdiff1d(np.arange(nf.U), [nf.QA, nf.QB])]).all()


def test_neg_inf_in_a_short_list_appears_and_counts():
    case, S, (ev, ei, ec) = solved("neg_inf_in_a_short_list")
    q, it = nf.HEAVY[0], nf.short_list_item()
    assert np.isneginf(S[q, it]) and not np.isnan(S).any()
    assert ec[q] == nf.LEFT
    assert ei[q, nf.LEFT - 1] == it and np.isneginf(ev[q, nf.LEFT - 1]) and np.isfinite(ev[q, :nf.LEFT - 1]).all()
    assert (ei[q, nf.LEFT:] == -1).all()
    assert ec[nf.HEAVY[1]] == nf.LEFT


@pytest.mark.parametrize("k", range(4))
def test_epilogue_makes_its_nans_after_the_dot_product(k):
    case, S, (ev, ei, ec) = solved("epilogue", k)
    dots = oracle.score_matrix(oracle.SCORE_NORMAL, case.P, case.Q)
    assert not np.isnan(dots).any() and np.isinf(dots[:, nf.SIG_I_ZERO]).all()
    assert np.isnan(S[nf.SIG_U_NAN]).all() and np.isnan(S[:, nf.SIG_I_NAN]).all()
    assert ec[nf.SIG_U_NAN] == 0
    assert not (ei == nf.SIG_I_NAN).any()
    if case.kind == oracle.SCORE_RUBI_BOTH:                  # (inf - c) * 0 = NaN
        assert np.isnan(S[:, nf.SIG_I_ZERO]).all() and not (ei == nf.SIG_I_ZERO).any()
    else:                                                    # inf - c * 0 * sig_u = inf: an ordinary score
        ok = np.arange(nf.U) != nf.SIG_U_NAN
        assert np.isinf(S[ok, nf.SIG_I_ZERO]).all()
        first = ok & np.isposinf(S[:, nf.SIG_I_ZERO]) & np.array([nf.SIG_I_ZERO not in set(m) for m in case.mask])
        assert first.sum() > 20 and (ei[first, 0] == nf.SIG_I_ZERO).all()


def test_all_nan_leaves_nobody_a_candidate():
    case, S, (ev, ei, ec) = solved("all_nan")
    assert np.isnan(S).all()
    assert (ec == 0).all() and (ei == -1).all() and np.isneginf(ev).all()


@pytest.mark.parametrize("d", [32, 128, 256])
def test_the_other_widths_keep_their_properties(d):
    for name in ("nan_item", "inf_query", "overflow_many"):
        case = nf.make(name, d)[0]
        S = oracle.score_matrix(case.kind, case.P, case.Q)
        ev, ei, ec = nf.expected_case(case)
        rv, ri, rc = nf.restated(S, nf.K, case.mask)
        assert np.array_equal(ei, ri) and np.array_equal(ec, rc) and np.array_equal(bits(ev), bits(rv))
        assert (ec == nf.K).mean() >= 0.9 and np.isnan(S).mean() < 0.05 and not np.isfinite(S).all()
        if name == "overflow_many":
            assert np.isposinf(ev[nf.QA]).all() and np.isposinf(ev[nf.QB, :5]).all()
