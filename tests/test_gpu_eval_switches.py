"""The Evaluator's switches against the oracle (-m gpu): every attribute that `macr_amd/evaluator.py` sets from the environment
(MACR_EVAL_GRAPH, _SEEDS, _OPTIMISTIC, _FOLD, _FOLD_PREP, _FILTER; tests/test_switches_cpu.py pins the parse), set on the
evaluator after construction, plus MACR_SWEEP_ONE_BY_ONE and MACR_LAZY_ADAM_MF, which are read per call.

The ops-level entry points of these arms have tests of their own (the prologues, metrics_mf_mean, first + repair round).  Here
it is the Evaluator's sequencing of them: which workspace is ready when, what a captured graph bakes in, what a repair round
finds when the prologue was not folded.  One problem -- d = 64, 5000 x 9000 tables, 600 sorted query users with 20 train and 5
held-out items each, SCORE_RUBI_BOTH at c = 30, Ks = [5, 20], a shape that ranks with thresholds -- and a second catalogue of 900
items that lists everything.  Every arm is driven through six evaluations: the first, two after a drift of ~1 % per row, one
after a jump (a new item table, in place), the one after it, one more drift; so every arm meets an unseeded round, seeded rounds,
a stale-seed repair and a back-off.  The six table states and their references are computed once and shared, unchanged:

    rankings   Evaluator.rank of the arm == oracle.score_topk on the HIP branch factors: ids, counts, score bits
    means      test_mf / test_lgcn of the arm == those of the plain evaluator (no seeds, no graph, default folds), bit for bit;
               with fold_metrics the mean is summed in another tree: rtol 1e-13 against the float64 mean of the oracle's per-query
               metrics_mf, the tolerance test_metrics_mf_mean_is_metrics_mf_then_the_mean_in_one_launch grants that kernel
"""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

KIND, C, KS = oracle.SCORE_RUBI_BOTH, 30.0, [5, 20]
D, N_USERS, N_ITEMS, U, N_SMALL = 64, 5000, 9000, 600, 900
STEPS = ("first", "drift", "drift", "jump", "after", "drift")
DEFAULT = dict(fold_prologue=True, fold_metrics=False, fold_prep=True, optimistic=True, use_seeds=True, use_graph=True, filter="f16")
ARMS = {
    "default": {},
    # every single departure
    "fold-m": dict(fold_prologue=False, fold_metrics=True),
    "fold-1": dict(fold_metrics=True),
    "fold-0": dict(fold_prologue=False),
    "prep0": dict(fold_prep=False),
    "optimistic0": dict(optimistic=False),
    "seeds0": dict(use_seeds=False),
    "graph0": dict(use_graph=False),
    "f32": dict(filter="f32"),
    # combined
    "fold-0+prep0+optimistic0": dict(fold_prologue=False, fold_prep=False, optimistic=False),
    "fold-1+graph0": dict(fold_metrics=True, use_graph=False),
    "fold-m+optimistic0": dict(fold_prologue=False, fold_metrics=True, optimistic=False),
    "f32+fold-0+graph0": dict(filter="f32", fold_prologue=False, use_graph=False),
    "prep0+seeds0": dict(fold_prep=False, use_seeds=False),
}
LGCN_ARMS = ("default", "fold-0+prep0+optimistic0", "graph0", "f32", "prep0")
SMALL_ARMS = ("default", "prep0", "fold-0", "optimistic0", "fold-1+graph0", "fold-0+prep0+optimistic0")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_evaluator(prob, arm, n_items=N_ITEMS):
    from macr_amd.evaluator import Evaluator
    ev = Evaluator(prob.mask[n_items], prob.gt[n_items], n_items, torch.device("cuda"))
    for name, value in dict(DEFAULT, **arm).items():       # every switch explicitly: whatever the environment of the run says
        setattr(ev, name, value)
    return ev


class Problem(object):
    """tables, queries, the six table states, and per (catalogue, state) the references -- computed once, then only read"""

    def __init__(self, ops):
        rs = np.random.RandomState(11)
        self.ops = ops
        P = (rs.standard_normal((N_USERS, D)) * 0.4).astype(np.float32)
        Q = (rs.standard_normal((N_ITEMS, D)) * 0.4).astype(np.float32)
        self.w, self.wu = dev((rs.standard_normal(D) * 0.3).astype(np.float32)), dev((rs.standard_normal(D) * 0.3).astype(np.float32))
        self.users = np.sort(rs.choice(N_USERS, U, replace=False)).astype(np.int32)
        self.uid = dev(self.users)
        self.mask, self.gt = {}, {}
        for n in (N_ITEMS, N_SMALL):
            self.mask[n] = [sorted(rs.choice(n, 20, replace=False).tolist()) for _ in range(U)]
            self.gt[n] = [sorted(rs.choice(n, 5, replace=False).tolist()) for _ in range(U)]
        # the six states: drift = every row moves by ~1 % of its length, jump = a new item table
        gen = torch.Generator(device="cuda").manual_seed(3)
        p, q = dev(P), dev(Q)
        self.states = []
        for step in STEPS:
            if step == "drift":
                q = q + torch.randn(q.shape, generator=gen, device="cuda") * 0.004
                p = p + torch.randn(p.shape, generator=gen, device="cuda") * 0.004
            elif step == "jump":
                q = torch.randn(q.shape, generator=gen, device="cuda") * 0.4
            self.states.append((p.clone(), q.clone()))
        # the buffers every evaluator reads (a captured graph bakes their addresses in); the small catalogue is its own table
        self.P, self.Q, self.Qs = p.clone(), q.clone(), q[:N_SMALL].clone()
        self.refs = {(n, k): self._reference(n, k) for n in (N_ITEMS, N_SMALL) for k in range(len(STEPS))}

    def load(self, k):
        self.P.copy_(self.states[k][0]); self.Q.copy_(self.states[k][1]); self.Qs.copy_(self.states[k][1][:N_SMALL])

    def items(self, n):
        return self.Q if n == N_ITEMS else self.Qs

    def _reference(self, n, k):
        ops = self.ops
        self.load(k)
        Q = self.items(n)
        sig_i = ops.branch_sigmoid(Q, self.w).cpu().numpy()
        sig_u = ops.branch_sigmoid(self.P, self.wu, self.uid).cpu().numpy()
        wv, wi, wc = oracle.score_topk(KIND, self.P.cpu().numpy()[self.users], Q.cpu().numpy(), max(KS), sig_u, sig_i, C,
                                       oracle.csr_from_lists(self.mask[n]))
        plain = make_evaluator(self, dict(use_seeds=False, use_graph=False), n)
        return {"rank": (wv, wi, wc),
                "mf": plain.test_mf(KIND, self.P, self.uid, Q, KS, self.w, self.wu, C),
                "lgcn": plain.test_lgcn(KIND, self.P, self.uid, Q, KS, self.w, self.wu, C),
                "mf_oracle_mean": oracle.metrics_mf(wi, wc, oracle.csr_from_lists(self.gt[n]), KS).mean(0)}


@pytest.fixture(scope="module")
def prob(ops):
    from macr_amd import _lib
    assert _lib.lib().macr_score_topk_uses_seeds(U, N_ITEMS, D) == 1           # thresholds, seeds and the repair round exist
    assert _lib.lib().macr_score_topk_uses_seeds(U, N_SMALL, D) == 0           # ... and here every item is listed
    return Problem(ops)


MF_KEYS = ("precision", "recall", "ndcg", "hit_ratio")


def assert_rank_is_oracle(got, want, where):
    (gv, gi, gc), (wv, wi, wc) = got, want
    assert np.array_equal(gi.cpu().numpy(), wi), where
    assert np.array_equal(gc.cpu().numpy(), wc), where
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), wv.view(np.uint32)), where


def assert_mf_means(got, ref, fold_metrics, where):
    if fold_metrics:
        got = np.stack([got[k] for k in MF_KEYS])
        np.testing.assert_allclose(got, ref["mf_oracle_mean"], rtol=1e-13, atol=0, err_msg=str(where))
    else:
        for k in MF_KEYS:
            assert np.array_equal(got[k], ref["mf"][k]), (where, k, got[k], ref["mf"][k])


def drive(prob, arm_name, n, flavour):
    """the six evaluations of one arm: its means through `ev`, its rankings through `rk` (an evaluator of the same arm: a
    ranking call in between would spend the evaluations of ev's back-off) -> ev, rk, [last_eval_info of ev per step]"""
    arm = dict(DEFAULT, **ARMS[arm_name])
    ev, rk = make_evaluator(prob, arm, n), make_evaluator(prob, arm, n)
    Q, infos, seeded_rank = prob.items(n), [], []
    for k, step in enumerate(STEPS):
        prob.load(k)
        ref, where = prob.refs[n, k], (arm_name, n, flavour, k, step)
        test = ev.test_mf if flavour == "mf" else ev.test_lgcn
        got = test(KIND, prob.P, prob.uid, Q, KS, prob.w, prob.wu, C)
        torch.cuda.synchronize()
        infos.append(ev.last_eval_info())
        print(where, infos[-1], {k_: np.asarray(v).tolist() for k_, v in got.items()})
        if flavour == "mf":
            assert_mf_means(got, ref, arm["fold_metrics"], where)
        else:
            for key in ("hr", "recall", "ndcg"):
                assert np.array_equal(got[key], ref["lgcn"][key]), (where, key, got[key], ref["lgcn"][key])
        assert_rank_is_oracle(rk.rank(KIND, prob.P, prob.uid, Q, max(KS), prob.w, prob.wu, C), ref["rank"], where)
        seeded_rank.append(rk.last_eval_info()["seeded"])
    print(arm_name, n, "rank seeded:", seeded_rank)
    return ev, rk, infos, seeded_rank


def assert_met_every_round(arm_name, infos, seeded_rank):
    """an unseeded round, seeded rounds that hold, a stale-seed repair, a back-off -- or, without seeds, none of it"""
    seeded = [bool(i["seeded"]) for i in infos]
    relisted = [i["query_blocks_relisted"] for i in infos]
    if not dict(DEFAULT, **ARMS[arm_name])["use_seeds"]:
        assert seeded == [False] * 6 and seeded_rank == [False] * 6, (seeded, seeded_rank)
        return
    assert seeded == [False, True, True, True, False, True], (arm_name, seeded, relisted)
    assert relisted[1:3] == [0, 0] and relisted[3] > 0 and relisted[5] == 0, (arm_name, relisted)
    assert all(i["exact_fallback"] == 0 for i in infos), (arm_name, infos)
    assert seeded_rank == [False, True, True, True, False, True], (arm_name, seeded_rank)


# ----------------------------------------------------------------------------- the arms
@pytest.mark.parametrize("arm_name", list(ARMS))
def test_mf_evaluations_of_every_arm(ops, prob, arm_name):
    arm = dict(DEFAULT, **ARMS[arm_name])
    ev, rk, infos, seeded_rank = drive(prob, arm_name, N_ITEMS, "mf")
    assert_met_every_round(arm_name, infos, seeded_rank)
    for name, value in arm.items():
        assert getattr(ev, name) == value, name                  # (nothing switched graph replay or a fold off under way)
    if not arm["use_graph"]:
        assert not ev._graphs and ev.fast_stats == {"fast": 0, "redone": 0}
    elif not arm["optimistic"]:
        # the complete sequence under graph replay: one graph seeded, one sampled, and no first-round bookkeeping
        assert ev.fast_stats == {"fast": 0, "redone": 0}
        assert len(ev._graphs) == 2
    elif arm["use_seeds"]:
        # first round seeded and sampled, and the repair round of the stale evaluation
        assert ev.fast_stats == {"fast": 5, "redone": 1}
        assert len(ev._graphs) == 3 and infos[3]["redone"] and not any(i["redone"] for k, i in enumerate(infos) if k != 3)
    else:
        assert ev.fast_stats == {"fast": 6, "redone": 0} and len(ev._graphs) == 1
    assert not rk._graphs                                        # (rank launches directly)


@pytest.mark.parametrize("arm_name", LGCN_ARMS)
def test_lgcn_evaluations(ops, prob, arm_name):
    ev, rk, infos, seeded_rank = drive(prob, arm_name, N_ITEMS, "lgcn")
    assert_met_every_round(arm_name, infos, seeded_rank)


@pytest.mark.parametrize("arm_name", SMALL_ARMS)
def test_catalogue_that_lists_everything(ops, prob, arm_name):
    """N = 900: no thresholds, so no seeds, no filter and no operand copies -- fold_prep stays out of the way (the plain
    prologue runs), no evaluation is ever seeded or redone, and the results are the oracle's all the same"""
    arm = dict(DEFAULT, **ARMS[arm_name])
    ev, rk, infos, seeded_rank = drive(prob, arm_name, N_SMALL, "mf")
    assert not any(i["seeded"] or i["query_blocks_relisted"] or i["exact_fallback"] or i["redone"] for i in infos), infos
    assert seeded_rank == [False] * 6 and not ev._seeds and not rk._seeds
    prob.load(5)
    ops.timing_begin()
    rk.rank(KIND, prob.P, prob.uid, prob.Qs, max(KS), prob.w, prob.wu, C)
    names = [n for n, _ in ops.timing_end(64)]
    assert "eval_prologue_prep" not in names and ("eval_prologue" in names) == arm["fold_prologue"], names
    assert not {"score_sample", "score_sample_b", "tau", "tau_seed"} & set(names), names


# ----------------------------------------------------------------------------- the settings take effect
@pytest.mark.parametrize("fold_prologue,fold_metrics,fold_prep,filt", [
    (True, False, True, "f16"), (True, False, False, "f16"), (False, False, True, "f16"), (False, True, True, "f16"),
    (True, True, True, "f16"), (True, False, True, "f32"), (False, True, False, "f32")])
def test_folds_select_their_launches(ops, prob, fold_prologue, fold_metrics, fold_prep, filt):
    """launched directly (use_graph = False), an unseeded and a seeded evaluation: the launch names say which fold ran"""
    arm = dict(fold_prologue=fold_prologue, fold_metrics=fold_metrics, fold_prep=fold_prep, filter=filt, use_graph=False)
    ev = make_evaluator(prob, arm)
    prob.load(0)
    for seeded in (False, True):
        ops.timing_begin()
        got = ev.test_mf(KIND, prob.P, prob.uid, prob.Q, KS, prob.w, prob.wu, C)
        names = [n for n, _ in ops.timing_end(64)]
        where = (arm, seeded, names)
        assert ev.last_eval_info()["seeded"] is seeded, where
        assert_mf_means(got, prob.refs[N_ITEMS, 0], fold_metrics, where)
        prep = fold_prologue and fold_prep and filt == "f16"
        assert ("eval_prologue_prep" in names) == prep, where
        assert ("eval_prologue" in names) == (fold_prologue and not prep), where
        assert ("branch_sigmoid" in names) == (not fold_prologue) and ("ws_init" in names) == (not fold_prologue), where
        if fold_metrics:
            assert "metrics_mf_mean" in names and "metrics_mf" not in names and "colmean" not in names, where
        else:
            assert "metrics_mf" in names and "colmean" in names and "metrics_mf_mean" not in names, where
        assert ("tau_seed" in names or "bf16_prep+tau_seed" in names) == seeded, where


# ----------------------------------------------------------------------------- MACR_SWEEP_ONE_BY_ONE
@pytest.mark.parametrize("use_graph", [True, False])
def test_sweep_one_by_one_equals_the_shared_pass(ops, prob, use_graph, monkeypatch):
    """MACR_SWEEP_ONE_BY_ONE=1 (read per call): test_mf_sweep over five values of c through the single evaluation, value by value,
    gives what the shared listing pass gives (groups of four and one), bit for bit; launched directly, the shared pass's operand
    copies (bf16_prep: a launch only the sweep entry point has) and its two listing passes are gone"""
    cs = [30.0, -5.0, 0.0, 12.5, 40.0]
    prob.load(1)
    out, names = {}, {}
    for one_by_one in (False, True):
        if one_by_one:
            monkeypatch.setenv("MACR_SWEEP_ONE_BY_ONE", "1")
        else:
            monkeypatch.delenv("MACR_SWEEP_ONE_BY_ONE", raising=False)
        ev = make_evaluator(prob, dict(use_graph=use_graph))
        if not use_graph:                                   # (no launch names of a capture: only the direct launches are timed)
            ops.timing_begin()
        out[one_by_one] = ev.test_mf_sweep(KIND, prob.P, prob.uid, prob.Q, KS, prob.w, prob.wu, cs)
        if not use_graph:
            names[one_by_one] = [n for n, _ in ops.timing_end(256)]
    monkeypatch.delenv("MACR_SWEEP_ONE_BY_ONE", raising=False)
    assert len(out[True]) == len(out[False]) == len(cs)
    for c, a, b in zip(cs, out[False], out[True]):
        for k in MF_KEYS:
            assert np.array_equal(a[k], b[k]), (c, k, a[k], b[k])
    assert any(not np.array_equal(out[True][0]["hit_ratio"], r["hit_ratio"]) for r in out[True][1:])       # c does change the ranking
    if not use_graph:
        assert "bf16_prep" in names[False] and names[False].count("score_stream_b") == 2, names[False]
        assert "bf16_prep" not in names[True] and names[True].count("score_stream_b") == len(cs), names[True]


# ----------------------------------------------------------------------------- MACR_LAZY_ADAM_MF
def test_lazy_adam_mf_from_the_environment(ops, monkeypatch):
    """MFState(..., lazy_period=None) takes its period from MACR_LAZY_ADAM_MF: six deferred steps are those of lazy_period=4 passed
    explicitly, bit for bit.  Batches without a repeated row and with at most eight backward blocks, as in
    test_mf_lazy_sequence_equals_the_dense_sequence_bit_for_bit: every atomic add lands on a zero, so a sequence is reproducible."""
    kind, n_users, n_items, d, B = ops.LOSS_RUBIBCEBOTH, 2000, 1500, 64, 128
    rs = np.random.RandomState(9)
    P = (rs.standard_normal((n_users, d)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    make = lambda **kw: ops.MFState(dev(P), dev(Q), dev(w), dev(wu), ops.make_hyper(1e-3, 1e-5, 1e-2, 1e-3, 1024), B, **kw)
    monkeypatch.delenv("MACR_LAZY_ADAM_MF", raising=False)
    explicit, unset = make(lazy_period=4), make(lazy_period=None)
    monkeypatch.setenv("MACR_LAZY_ADAM_MF", "4")
    from_env, argument_wins = make(lazy_period=None), make(lazy_period=2)
    monkeypatch.delenv("MACR_LAZY_ADAM_MF", raising=False)
    assert (explicit.lazy_period, unset.lazy_period, from_env.lazy_period, argument_wins.lazy_period) == (4, None, 4, 2)
    for step in range(6):
        u = rs.choice(n_users, B, replace=False).astype(np.int32)
        ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)
        b = [dev(a) for a in (u, ij[:B], ij[B:])]
        la, lb = explicit.step(kind, *b, defer=True).clone(), from_env.step(kind, *b, defer=True).clone()
        assert from_env._seq_lazy is not None and from_env._seq_lazy.period == 4 and explicit._seq_lazy.period == 4
        assert torch.equal(la, lb), (step, la, lb)
    explicit.flush(); from_env.flush()
    for name in ("P", "Q", "w", "wu", "mP", "vP", "mQ", "vQ", "mw", "vw", "mwu", "vwu", "adam_pow"):
        assert torch.equal(getattr(from_env, name), getattr(explicit, name)), name
    assert not from_env.tP.any() and not from_env.tQ.any() and not from_env.gP.any() and not from_env.gQ.any()
    assert not torch.equal(from_env.P, dev(P))                               # (the steps did train)
