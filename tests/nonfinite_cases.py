"""Tables with NaN, infinite and overflowing scores for the fused ranking (macr_score_topk, macr_score_topk_sweep), and the result
the rule of include/macr_hip.h asks for on them.

The rule: a (query, item) pair whose fp32 score -- the k-ascending fma chain, then the kind's epilogue -- is NaN is NO CANDIDATE,
exactly as if the query masked the item.  +inf and -inf are ordinary scores: +inf ranks first, an unmasked item scoring -inf is a
candidate, counts and leaves as (-inf, id); ties, also at +-inf, go to the lower id.  No NaN ever appears among the values; a query
with no candidate left has count 0 and K slots of (-inf, -1).

expected() states that with the oracle alone: oracle.score_matrix says which scores are NaN, those ids join the query's mask, and
oracle.score_topk ranks the rest.  (orc_score_topk by itself inserts a NaN score while a list is short: it does not carry the rule.)
restated() says the same with numpy only; tests/test_nonfinite_cases_cpu.py holds the two to each other and every case to the
property it is named for, tests/test_gpu_nonfinite.py runs the kernels against expected().

Every case is a small edit of one base problem: U = 300 queries (two blocks of 256: a damaged query of block 0 must leave block 1
alone), N = 4000 items (above the list-everything limit), K = 20, Poisson(10) masks, two queries whose mask leaves 4 candidates.
"""
import collections

import numpy as np

import oracle

U, N, D, K = 300, 4000, 64, 20
HEAVY = (5, 270)                  # queries whose mask leaves 4 candidates, one per block of 256 queries
LEFT = 4
QA, QB = 7, 200                   # the damaged query rows (blocks 0 and 0; QB mirrors QA in the overflow cases)
COL, COL2 = 3, 9                  # the damaged columns
BIG_U, BIG_I = 1.8e19, 2.0e19     # finite, with a product beyond FLT_MAX (3.4e38): the fma chain overflows to +-inf
NAN, INF = np.float32(np.nan), np.float32(np.inf)

Case = collections.namedtuple("Case", "name kind c P Q sig_u sig_i mask")

NAMES = ("nan_query", "nan_item", "inf_query", "inf_item", "inf_minus_inf", "overflow_many", "overflow_few",
         "neg_inf_in_a_short_list", "epilogue", "all_nan")
EPILOGUE_KINDS = (oracle.SCORE_RUBI_BOTH, oracle.SCORE_DIRECT_MINUS_BOTH)
EPILOGUE_CS = (40.0, -2.5)
NAN_ITEM, INF_ITEM_POS, INF_ITEM_NEG = 11, 11, 12
ZERO_ITEMS = (100, 101, 2500)     # inf_query: an exact 0.0 under the query's +inf (0 * inf = NaN)
SIG_I_NAN, SIG_I_ZERO, SIG_U_NAN = 17, 18, 9

_base_cache = {}


def base(d=D):
    """(P, Q, sig_u, sig_i, mask lists) of the undamaged problem at embedding width d -- the same arrays on every call: copy before
    editing"""
    if d not in _base_cache:
        rs = np.random.RandomState(7700 + d)
        P = (rs.standard_normal((U, d)) * 0.4).astype(np.float32)
        Q = (rs.standard_normal((N, d)) * 0.4).astype(np.float32)
        sig_u = (1.0 / (1.0 + np.exp(-rs.standard_normal(U)))).astype(np.float32)
        sig_i = (1.0 / (1.0 + np.exp(-rs.standard_normal(N)))).astype(np.float32)
        mask = []
        for q in range(U):
            k = N - LEFT if q in HEAVY else min(int(rs.poisson(10)), N)
            mask.append(sorted(rs.choice(N, size=k, replace=False).tolist()))
        for a in (P, Q, sig_u, sig_i):
            a.setflags(write=False)
        _base_cache[d] = (P, Q, sig_u, sig_i, mask)
    return _base_cache[d]


def overflow_rows(n_pos, n_neg=5):
    """item rows of the overflow cases: n_pos hold +BIG_I in COL, n_neg hold -BIG_I (spread over the catalogue, fixed)"""
    rows = np.random.RandomState(99).permutation(N)[:n_pos + n_neg]
    return np.sort(rows[:n_pos]), np.sort(rows[n_pos:])


def short_list_item(d=D):
    """the candidate of HEAVY[0] that neg_inf_in_a_short_list sends to -inf: the second of her 4 unmasked ids"""
    mask = base(d)[4]
    return sorted(set(range(N)) - set(mask[HEAVY[0]]))[1]


def make(name, d=D):
    """-> list of Case (one, except for `epilogue`: a kind x c grid on the same tables)"""
    P0, Q0, su0, si0, mask = base(d)
    P, Q, sig_u, sig_i = P0.copy(), Q0.copy(), su0.copy(), si0.copy()
    kind, cs = oracle.SCORE_NORMAL, (0.0,)
    if name == "nan_query":
        P[QA, COL] = NAN
    elif name == "nan_item":
        Q[NAN_ITEM, 5] = NAN
    elif name == "inf_query":
        P[QA, COL] = INF
        Q[list(ZERO_ITEMS), COL] = 0.0
    elif name == "inf_item":
        Q[INF_ITEM_POS, 5] = INF
        Q[INF_ITEM_NEG, COL2] = -INF
    elif name == "inf_minus_inf":
        Q[NAN_ITEM, 5] = INF
        Q[NAN_ITEM, COL2] = -INF
    elif name in ("overflow_many", "overflow_few"):
        pos, neg = overflow_rows(30 if name == "overflow_many" else 3)
        P[QA, COL], P[QB, COL] = BIG_U, -BIG_U
        Q[pos, COL], Q[neg, COL] = BIG_I, -BIG_I
    elif name == "neg_inf_in_a_short_list":
        Q[short_list_item(d), COL] = -INF if P[HEAVY[0], COL] > 0 else INF       # -inf for HEAVY[0], +-inf for the others
    elif name == "epilogue":
        sig_i[SIG_I_NAN] = NAN
        sig_i[SIG_I_ZERO] = 0.0
        Q[SIG_I_ZERO, COL] = INF                                                 # dot product +-inf by the sign of P[q, COL]
        sig_u[SIG_U_NAN] = NAN
        return [Case("epilogue", k, c, P, Q, sig_u, sig_i, mask) for k in EPILOGUE_KINDS for c in EPILOGUE_CS]
    elif name == "all_nan":
        Q[:, 5] = NAN
    else:
        raise KeyError(name)
    return [Case(name, kind, c, P, Q, sig_u, sig_i, mask) for c in cs]


def with_sigs(case):
    """the Case's (sig_u, sig_i) as the entry points want them: None for SCORE_NORMAL"""
    return (None, None) if case.kind == oracle.SCORE_NORMAL else (case.sig_u, case.sig_i)


def nan_extended_mask(kind, P, Q, sig_u, sig_i, c, mask_lists, item_offset=0):
    """mask lists plus, per query, the (global) ids whose score is NaN; also returns the score matrix"""
    S = oracle.score_matrix(kind, P, Q, sig_u, sig_i, c)
    nan = np.isnan(S)
    rows_with = np.flatnonzero(nan.any(axis=1))
    ext = list(mask_lists)
    for q in rows_with:
        ext[q] = sorted(set(mask_lists[q]) | set((np.flatnonzero(nan[q]) + item_offset).tolist()))
    return ext, S


def expected(kind, P, Q, K, sig_u, sig_i, c, mask_lists, item_offset=0):
    """(val (U,K) f32, idx (U,K) i32, cnt (U,) i32): the oracle's ranking with every NaN-scoring pair masked"""
    ext, _ = nan_extended_mask(kind, P, Q, sig_u, sig_i, c, mask_lists, item_offset)
    return oracle.score_topk(kind, P, Q, K, sig_u, sig_i, c, oracle.csr_from_lists(ext), item_offset)


def expected_case(case, K=K):
    su, si = with_sigs(case)
    return expected(case.kind, case.P, case.Q, K, su, si, case.c, case.mask)


def restated(S, K, mask_lists, item_offset=0):
    """the rule in numpy on a score matrix: candidates = unmasked and not NaN, order = (score descending, id ascending)"""
    Un, Nn = S.shape
    val = np.full((Un, K), -np.inf, np.float32)
    idx = np.full((Un, K), -1, np.int32)
    cnt = np.zeros(Un, np.int32)
    for q in range(Un):
        ok = ~np.isnan(S[q])
        m = np.asarray(mask_lists[q], np.int64) - item_offset
        m = m[(m >= 0) & (m < Nn)]
        ok[m] = False
        ids = np.flatnonzero(ok)
        order = ids[np.lexsort((ids, -S[q, ids].astype(np.float64)))][:K]
        cnt[q] = len(order)
        val[q, :len(order)] = S[q, order]
        idx[q, :len(order)] = order + item_offset
    return val, idx, cnt
