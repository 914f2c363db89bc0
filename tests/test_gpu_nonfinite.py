"""The fused ranking on NaN, infinite and overflowing scores (-m gpu): macr_score_topk under every filter, round and K, item
shards, the c sweep and the Evaluator against tests/nonfinite_cases.py::expected() -- the rule of include/macr_hip.h: a NaN score
is no candidate, +-inf are ordinary scores, ties go to the lower id, no NaN among the values, (-inf, -1) pads a short list.

Every comparison is exact: ids, counts, and values as uint32.  Which path pays for such input (stats) is recorded, not asserted.
tests/test_nonfinite_cases_cpu.py holds expected() to a numpy restatement of the rule and every case to what it is named for.
"""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
import oracle

gpu = pytest.mark.gpu
pytestmark = gpu

MODES = ("sampled", "seeded", "first round + repair round")
VARIANTS = [(name, k) for name in nf.NAMES for k in range(4 if name == "epilogue" else 1)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


@pytest.fixture(params=["f32", "bf16", "f16"])
def eval_filter(request, ops, monkeypatch):
    """run the test once per candidate filter of the listing pass (include/macr_hip.h MACR_EVAL_FILTER_*): the ranking
    must be the fp32 ranking bit for bit either way"""
    monkeypatch.setenv("MACR_EVAL_FILTER", request.param)       # what an Evaluator created by the test picks up
    ops.set_eval_filter(request.param)
    yield request.param
    ops.set_eval_filter("env")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the base tables are read-only)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_want, _tables, _masks = {}, {}, {}


def case_of(name, k=0, d=nf.D):
    return nf.make(name, d)[k]


def want_of(name, k=0, d=nf.D, K=nf.K):
    """expected() of a case: computed once, shared by every test that needs it, never written to"""
    key = (name, k, d, K)
    if key not in _want:
        _want[key] = nf.expected_case(case_of(name, k, d), K)
        for a in _want[key]:
            a.setflags(write=False)
    return _want[key]


def mask_on_device(ops, d=nf.D):
    if d not in _masks:
        _masks[d] = ops.CSR.from_lists(nf.base(d)[4], "cuda")
    return _masks[d]


def tables_on_device(case, d=nf.D):
    su, si = nf.with_sigs(case)
    return dev(case.P), dev(case.Q), dev(su), dev(si)


def base_seeds(ops, case, K, d=nf.D):
    """seed_out of a call on the UNDAMAGED tables (same kind, c, K, filter): seeds that now name NaN / +-inf scoring ids"""
    P, Q, sig_u, sig_i, _ = nf.base(d)
    su, si = (None, None) if case.kind == oracle.SCORE_NORMAL else (sig_u, sig_i)
    seeds = torch.full((nf.U, ops.SEED_WIDTH), -1, dtype=torch.int32, device="cuda")
    ops.score_topk(case.kind, dev(P), None, dev(Q), K, dev(su), dev(si), case.c, mask_on_device(ops, d), seed_out=seeds)
    return seeds


def same(v, ix, want, tag):
    wv, wi, wc = want
    gv, gi = v.cpu().numpy(), ix.cpu().numpy()
    assert not np.isnan(gv).any(), tag
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert bad.size == 0, (tag, "queries", bad[:8].tolist(), "got", gi[bad[0]].tolist(), "want", wi[bad[0]].tolist())
    badv = np.flatnonzero((bits(gv) != bits(wv)).any(axis=1))
    assert badv.size == 0, (tag, "queries", badv[:8].tolist(), "got", gv[badv[0]].tolist(), "want", wv[badv[0]].tolist())
    assert np.array_equal((gi >= 0).sum(axis=1), wc), tag


def ranked(ops, case, K, mode, record_property, d=nf.D, want=None, tag=None):
    """one ranking of `case` in `mode`, checked against `want`: the result, seed_out[:, :K] == out_idx, the merged count"""
    Pd, Qd, sud, sid = tables_on_device(case, d)
    mcsr = mask_on_device(ops, d)
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    seeds_out = torch.full((nf.U, ops.SEED_WIDTH), -7, dtype=torch.int32, device="cuda")
    seed = base_seeds(ops, case, K, d) if mode == "seeded" else None
    if mode == MODES[2]:
        v, ix = ops.score_topk(case.kind, Pd, None, Qd, K, sud, sid, case.c, mcsr, seed_out=seeds_out, stats=stats, first_round=True)
        record_property("stats_first_round", stats.cpu().numpy().tolist())
        ops.score_topk(case.kind, Pd, None, Qd, K, sud, sid, case.c, mcsr, seed_out=seeds_out, stats=stats,
                       repair_of=(v, ix, ops._topk_ws_cache[v.device]))
    else:
        v, ix = ops.score_topk(case.kind, Pd, None, Qd, K, sud, sid, case.c, mcsr, seed=seed, seed_out=seeds_out, stats=stats)
    record_property("stats", stats.cpu().numpy().tolist())
    tag = tag or (case.name, case.kind, case.c, K, mode)
    same(v[0], ix[0], want, tag)
    if K <= ops.SEED_WIDTH and ops._lib.lib().macr_score_topk_uses_seeds(nf.U, nf.N, d):
        assert np.array_equal(seeds_out[:, :K].cpu().numpy(), want[1]), tag          # the header's promise
    mv, mi, mc = ops.topk_merge(v, ix)
    same(mv, mi, want, tag)
    assert np.array_equal(mc.cpu().numpy(), want[2]), tag


# ---- 1. every case x filter x mode at K = 20; K = 1 and 32 on two of them ------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,k", VARIANTS)
def test_every_case_ranks_by_the_rule(ops, eval_filter, name, k, mode, record_property):
    """bf16_prep_block's "NaN row: margin +inf", the fp16 filter's "operand is CLAMPED ... norm reported as +inf", k_select_b's
    "a NaN score is no candidate", tau_seed_block's "NaN: no bound from this seed", the kNone poisoning of k_score_topk /
    k_score_stream and filter_margin_h's `m == m ? m : INFINITY` (macr_amd/csrc/eval_kernels.hip) are what these cases run"""
    ranked(ops, case_of(name, k), nf.K, mode, record_property, want=want_of(name, k))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("name", ["nan_item", "overflow_many"])
def test_the_smallest_and_largest_fused_K(ops, eval_filter, name, K, mode, record_property):
    ranked(ops, case_of(name), K, mode, record_property, want=want_of(name, K=K))


# ---- 2. the other embedding widths: operand copies, norms and clamps are per-d code -------------------------------------------
@pytest.mark.parametrize("d", [32, 128, 256])
@pytest.mark.parametrize("name", ["nan_item", "inf_query", "overflow_many"])
def test_the_other_widths(ops, eval_filter, name, d, record_property):
    for mode in MODES[:2]:
        ranked(ops, case_of(name, 0, d), nf.K, mode, record_property, d=d, want=want_of(name, 0, d))


# ---- 3. the wide ranking (K > 32): k_score_matrix + k_topk_scores_wide ---------------------------------------------------------
@pytest.mark.parametrize("K", [50, 128])
@pytest.mark.parametrize("name,k", [v for v in VARIANTS if v[0] in ("nan_query", "nan_item", "inf_minus_inf", "overflow_many",
                                                                    "epilogue", "all_nan")])
def test_the_wide_ranking_drops_nan_scores_too(ops, eval_filter, name, k, K, record_property):
    """k_topk_scores_wide keyed every score by its bit pattern, under which a positive NaN sorts above +inf: the same tables
    ranked a NaN-scoring item FIRST at K = 50 and nowhere at K = 20"""
    ranked(ops, case_of(name, k), K, "sampled", record_property, want=want_of(name, k, K=K))


# ---- 4. item shards, merged -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [20, 50])
@pytest.mark.parametrize("name", ["nan_item", "overflow_many", "neg_inf_in_a_short_list"])
def test_three_item_shards_merge_to_the_whole_catalogue(ops, eval_filter, name, K):
    case = case_of(name)
    Pd, Qd, _, _ = tables_on_device(case)
    mcsr = mask_on_device(ops)
    bounds = [0, 1333, 2667, nf.N]
    vs, ixs = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        v, ix = ops.score_topk(case.kind, Pd, None, Qd[lo:hi].contiguous(), K, mask=mcsr, item_offset=lo)
        mv, mi, _ = ops.topk_merge(v, ix)
        assert not torch.isnan(mv).any()
        vs.append(mv); ixs.append(mi)
    gv, gi, gc = ops.topk_merge(torch.stack(vs), torch.stack(ixs))
    want = want_of(name, K=K)
    same(gv, gi, want, (name, K))
    assert np.array_equal(gc.cpu().numpy(), want[2])


# ---- 5. the c sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", nf.EPILOGUE_KINDS)
def test_the_c_sweep_on_the_epilogue_tables(ops, eval_filter, kind):
    base = [c for c in nf.make("epilogue") if c.kind == kind][0]
    Pd, Qd, sud, sid = tables_on_device(base)
    cs = [0.0, 20.0, 40.0]
    v, ix = ops.score_topk_sweep(kind, Pd, None, Qd, nf.K, sud, sid, dev(np.asarray(cs, np.float32)), mask_on_device(ops))
    for g, c in enumerate(cs):
        want = nf.expected(kind, base.P, base.Q, nf.K, base.sig_u, base.sig_i, c, base.mask)
        same(v[g], ix[g], want, (kind, c))


# ---- 6. the score entry points agree on the class of every score ---------------------------------------------------------------
@pytest.mark.parametrize("name,k", VARIANTS)
def test_score_matrix_and_rank_positions_see_the_same_classes(ops, name, k):
    """macr_score_matrix has NaN exactly where the oracle has it and the oracle's bits elsewhere (+-inf included); every
    expected top-K id has the position it holds in the list and every NaN-scoring id has none (macr_rank_positions' rule,
    already pinned by tests/test_gpu_rank_positions.py): the top-K rule and the position rule are one"""
    case = case_of(name, k)
    su, si = nf.with_sigs(case)
    Pd, Qd, sud, sid = tables_on_device(case)
    S = oracle.score_matrix(case.kind, case.P, case.Q, su, si, case.c)
    got = ops.score_matrix(case.kind, Pd, None, Qd, sud, sid, case.c).cpu().numpy()
    nan = np.isnan(S)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(S)[~nan])
    _, wi, wc = want_of(name, k)
    pairs, pos = [], []
    for q in range(nf.U):
        where = {int(i): r for r, i in enumerate(wi[q, :wc[q]])}
        free = np.setdiff1d(np.flatnonzero(nan[q]), case.mask[q])[:5]          # (a few of a NaN row's 4000)
        for i in free:
            where[int(i)] = -1
        row = sorted(where)
        pairs.append(row)
        pos.extend(where[i] for i in row)
    got_pos = ops.rank_positions(case.kind, Pd, None, Qd, ops.CSR.from_lists(pairs, "cuda"), sud, sid, case.c, mask_on_device(ops))
    assert np.array_equal(got_pos.cpu().numpy(), np.asarray(pos, np.int32))


# ---- 7. through the Evaluator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ks", [[20], [20, 50]])
def test_the_evaluator_on_nan_and_overflowing_tables(ops, eval_filter, Ks):
    """test_mf twice (the second call is the graph replay, seeded by the first) and test_mf_sweep on tables with a NaN item row and
    overflowing products: the metrics of the expected lists, at the rtol test_metrics_and_evaluator_with_wide_Ks uses"""
    from macr_amd.evaluator import Evaluator
    a, b = case_of("nan_item"), case_of("overflow_many")
    P, Q, mask = b.P.copy(), b.Q.copy(), b.mask
    Q[nf.NAN_ITEM] = a.Q[nf.NAN_ITEM]
    rs = np.random.RandomState(31)
    w, wu = (rs.standard_normal(nf.D) * 0.3).astype(np.float32), (rs.standard_normal(nf.D) * 0.3).astype(np.float32)
    gt = [sorted(rs.choice(nf.N, rs.randint(1, 30), replace=False).tolist()) for _ in range(nf.U)]
    kind, c = oracle.SCORE_RUBI_BOTH, 40.0
    uid, Pd, Qd, wd, wud = dev(np.arange(nf.U, dtype=np.int32)), dev(P), dev(Q), dev(w), dev(wu)
    sig_i = ops.branch_sigmoid(Qd, wd).cpu().numpy()
    sig_u = ops.branch_sigmoid(Pd, wud, uid).cpu().numpy()
    gcsr = oracle.csr_from_lists(gt)
    ev = Evaluator(mask, gt, nf.N, torch.device("cuda"))

    def metrics(cc):
        _, wi, wc = nf.expected(kind, P, Q, max(Ks), sig_u, sig_i, cc, mask)
        return oracle.metrics_mf(wi, wc, gcsr, Ks).mean(0)

    want = metrics(c)
    for rep in range(2):
        got = ev.test_mf(kind, Pd, uid, Qd, Ks, wd, wud, c)
        for row, key in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            np.testing.assert_allclose(got[key], want[row], rtol=1e-12, err_msg="%s, call %d" % (key, rep))
    cs = [0.0, 20.0, 40.0]
    for cc, got in zip(cs, ev.test_mf_sweep(kind, Pd, uid, Qd, Ks, wd, wud, cs)):
        want = metrics(cc)
        for row, key in enumerate(("precision", "recall", "ndcg", "hit_ratio")):
            np.testing.assert_allclose(got[key], want[row], rtol=1e-12, err_msg="%s, sweep c=%g" % (key, cc))
