"""Worker of tests/test_gpu_switch_children.py: the arms of the native code that only an environment switch selects, each
latched by a `static const` at first use and therefore run in a process of its own that has the switch in its environment.
Runs the arm against the CPU oracle, collects the launch names that prove the arm ran, prints one JSON verdict line.

    python tests/switch_worker.py stage_listed0 d32-hot | d32-flat | d256-hot | d256-flat      MACR_STAGE_LISTED=0
    python tests/switch_worker.py staging1                                                     MACR_STAGING=1
    python tests/switch_worker.py f32_sample                                                   MACR_EVAL_F32_SAMPLE=f32
    python tests/switch_worker.py f32_sample_off                                               (the variable unset)
    python tests/switch_worker.py lgcn_dense                                                   MACR_LGCN_DENSE=1

The worker refuses an environment that is not its setting's: a verdict says which arm it is about.
"""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle  # noqa: E402

ENV = {"stage_listed0": {"MACR_STAGE_LISTED": "0"}, "staging1": {"MACR_STAGING": "1"}, "f32_sample": {"MACR_EVAL_F32_SAMPLE": "f32"},
       "f32_sample_off": {}, "lgcn_dense": {"MACR_LGCN_DENSE": "1"}}
STAGE_LISTED_PARTS = {"d32-hot": (32, True), "d32-flat": (32, False), "d256-hot": (256, True), "d256-flat": (256, False)}
LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 1024


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def timed(ops, call, max_n=128):
    """(what call() returned, the launch names of the call in order)"""
    ops.timing_begin()
    out = call()
    return out, [n for n, _ in ops.timing_end(max_n)]


def assert_clean(state, where):
    """the ABI's scratch invariant: gradient scratch and row flags are zero again after a complete step"""
    assert float(state.gP.abs().max()) == 0.0 and float(state.gQ.abs().max()) == 0.0, where
    assert int(state.tP.sum()) == 0 and int(state.tQ.sum()) == 0, where


# ----------------------------------------------------------------------------- MACR_STAGE_LISTED=0
def stage_listed0(ops, res, part):
    """B = 20000 (staged path, a step complete in one call) with the gradient rows staged in batch order and found through the
    sorted list: ref_sort -> seg_index (k_seg_scan) -> seg_sum with the list's values -> the indexed Adam pass reading them.
    The batches of test_large_batch_indexed_adam_equals_segment_reduce (hot: Zipf positives, one item with thousands of
    references -- k_seg_sum's work items; flat: no row above 16 references -- every row summed by the Adam pass itself), three
    steps against oracle.mf_train_step with the assertions and tolerances of test_mf_large_batch_staged_path_matches_oracle."""
    d, hot = STAGE_LISTED_PARTS[part]
    n_users, n_items, B = 30000, (9000 if hot else 60000), 20000
    for kind_name in ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH"):
        kind, tag = getattr(oracle, kind_name), "%s %s" % (kind_name, part)
        rs = np.random.RandomState(5 + d + kind)
        P = (rs.standard_normal((n_users, d)) * 0.1).astype(np.float32)
        Q = (rs.standard_normal((n_items, d)) * 0.1).astype(np.float32)
        w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
        st = oracle.AdamState([P.shape, Q.shape, (d,), (d,)])
        Po, Qo, wo, wuo = P.copy(), Q.copy(), w.copy(), wu.copy()
        state = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), ops.make_hyper(LR, DECAY, ALPHA, BETA, BS), B)
        for t in range(3):
            u = rs.randint(0, n_users, B).astype(np.int32)
            i = ((rs.zipf(1.2, B) % n_items) if hot else rs.randint(0, n_items, B)).astype(np.int32)
            j = rs.randint(0, n_items, B).astype(np.int32)
            most = max(np.bincount(np.concatenate([i, j])).max(), np.bincount(u).max())
            assert most > 1000 if hot else most <= 16, (tag, most)
            want = oracle.mf_train_step(kind, u, i, j, Po, Qo, wo, wuo, st, LR, DECAY, ALPHA, BETA, BS)
            got, names = timed(ops, lambda: state.step(kind, dev(u), dev(i), dev(j)).cpu().numpy().copy())
            res["names"]["%s step %d" % (tag, t)] = names
            for name in ("ref_sort", "seg_index", "seg_sum", "adam_indexed"):
                assert name in names, (tag, t, name, names)
            assert "ref_place" not in names, (tag, t, names)
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg="%s step %d" % (tag, t))
            if t == 0:
                for name, gm, om in (("P", state.mP, st.m[0]), ("Q", state.mQ, st.m[1])):
                    np.testing.assert_allclose(gm.cpu().numpy() / 0.1, om / 0.1, rtol=2e-4, atol=2e-6 * np.abs(om / 0.1).max(),
                                               err_msg="%s d%s" % (tag, name))
            assert_clean(state, (tag, t))
        for name, mine, theirs in (("P", state.P, Po), ("Q", state.Q, Qo), ("mP", state.mP, st.m[0]), ("mQ", state.mQ, st.m[1]),
                                   ("vP", state.vP, st.v[0]), ("vQ", state.vQ, st.v[1])):
            np.testing.assert_allclose(mine.cpu().numpy(), theirs, rtol=1e-3, atol=1e-6 + 1e-4 * np.abs(theirs).max(),
                                       err_msg="%s %s" % (tag, name))
        res["losses"][tag] = got.tolist()


# ----------------------------------------------------------------------------- MACR_STAGING=1
STAGING_SHAPES = [(64, 32, 100, 40), (96, 64, 300, 50), (257, 64, 300, 50), (1024, 256, 3000, 900)]      # B, d, n_users, n_items


def check_staged_names(names, where):
    assert "ref_sort" in names and "batch_sort" not in names, (where, names)


def staging1_bce(ops, res, kind_name, B, d, n_users, n_items):
    """the body of test_gpu_ops.py::test_mf_train_step_matches_oracle, with its tolerances, on the staged path"""
    from test_gpu_ops import make_problem
    kind, tag = getattr(oracle, kind_name), "%s B%d d%d" % (kind_name, B, d)
    P, Q, w, wu, u, i, j = make_problem(B + d, n_users, n_items, d, B)
    st = oracle.AdamState([P.shape, Q.shape, (d,), (d,)])
    Po, Qo, wo, wuo = P.copy(), Q.copy(), w.copy(), wu.copy()
    state = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), ops.make_hyper(LR, DECAY, ALPHA, BETA, BS), B)
    rs = np.random.RandomState(9)
    for t in range(3):
        if t:
            u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
            i = rs.randint(0, n_items, B).astype(np.int32)
            j = rs.randint(0, n_items, B).astype(np.int32)
        want = oracle.mf_train_step(kind, u, i, j, Po, Qo, wo, wuo, st, LR, DECAY, ALPHA, BETA, BS)
        got, names = timed(ops, lambda: state.step(kind, dev(u), dev(i), dev(j)).cpu().numpy().copy())
        check_staged_names(names, (tag, t))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg="%s step %d" % (tag, t))
        if t == 0:
            res["names"][tag] = names
            for name, gm, om in (("P", state.mP, st.m[0]), ("Q", state.mQ, st.m[1])):
                g_hip, g_orc = gm.cpu().numpy() / 0.1, om / 0.1
                np.testing.assert_allclose(g_hip, g_orc, rtol=2e-4, atol=1e-6 * np.abs(g_orc).max(), err_msg="%s d%s" % (tag, name))
            if kind != oracle.LOSS_NORMALBCE:
                np.testing.assert_allclose(state.mw.cpu().numpy(), st.m[2], rtol=2e-4, atol=1e-6 * np.abs(st.m[2]).max(), err_msg=tag)
            if kind == oracle.LOSS_RUBIBCEBOTH:
                np.testing.assert_allclose(state.mwu.cpu().numpy(), st.m[3], rtol=2e-4, atol=1e-6 * np.abs(st.m[3]).max(), err_msg=tag)
        for name, mine, theirs in (("P", state.P, Po), ("Q", state.Q, Qo), ("w", state.w, wo), ("wu", state.wu, wuo)):
            np.testing.assert_allclose(mine.cpu().numpy(), theirs, rtol=0, atol=2e-3 * LR * (t + 1), err_msg="%s %s step %d" % (tag, name, t))
    for name, mine, theirs in (("mP", state.mP, st.m[0]), ("mQ", state.mQ, st.m[1]), ("vP", state.vP, st.v[0]), ("vQ", state.vQ, st.v[1])):
        np.testing.assert_allclose(mine.cpu().numpy(), theirs, rtol=1e-4, atol=2e-6 * np.abs(theirs).max(), err_msg="%s %s" % (tag, name))
    assert_clean(state, tag)
    np.testing.assert_allclose(state.adam_pow.cpu().numpy(), st.power, rtol=1e-6)
    if kind == oracle.LOSS_NORMALBCE:            # branch vectors get no gradient -> bitwise untouched
        assert np.array_equal(state.w.cpu().numpy(), w) and np.array_equal(state.wu.cpu().numpy(), wu), tag
    if kind == oracle.LOSS_RUBIBCE:              # no user branch
        assert np.array_equal(state.wu.cpu().numpy(), wu), tag
    res["losses"][tag] = got.tolist()


def staging1_bpr(ops, res, kind_name, B, d, n_users, n_items):
    """the same body for the two BPR kinds, against their float64 restatements (tests/bpr_ref.py, tests/rubi_bpr_ref.py) and
    bpr_ref.Adam: losses 1e-5 relative, the first step's gradient and the tables (0.2 % of a step per step) as in
    test_mf_train_step_matches_oracle"""
    import bpr_ref
    import rubi_bpr_ref
    from test_gpu_ops import make_problem
    rubi = kind_name == "LOSS_RUBIBPR"
    kind, tag = getattr(ops, kind_name), "%s B%d d%d" % (kind_name, B, d)
    P, Q, w, wu, u, i, j = make_problem(B + d, n_users, n_items, d, B)
    ref = bpr_ref.Adam([P, Q, w] if rubi else [P, Q], LR)
    state = ops.MFState(dev(P), dev(Q), dev(w), dev(wu), ops.make_hyper(LR, DECAY, ALPHA, BETA, BS), B)
    rs = np.random.RandomState(9)
    for t in range(3):
        if t:
            u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
            i = rs.randint(0, n_items, B).astype(np.int32)
            j = rs.randint(0, n_items, B).astype(np.int32)
        if rubi:
            want = rubi_bpr_ref.mf_rubi_bpr(ref.params[0], ref.params[1], ref.params[2], u, i, j, ALPHA, DECAY, BS)
        else:
            want = bpr_ref.mf_bpr(ref.params[0], ref.params[1], u, i, j, DECAY, BS)
        got, names = timed(ops, lambda: state.step(kind, dev(u), dev(i), dev(j)).cpu().numpy().copy())
        check_staged_names(names, (tag, t))
        np.testing.assert_allclose(got, want[:3], rtol=1e-5, atol=0, err_msg="%s step %d" % (tag, t))
        if t == 0:
            res["names"][tag] = names
            grads = (("P", state.mP, want[3]), ("Q", state.mQ, want[4])) + ((("w", state.mw, want[5]),) if rubi else ())
            for name, gm, g_ref in grads:
                np.testing.assert_allclose(gm.cpu().numpy() / 0.1, g_ref, rtol=2e-4, atol=1e-6 * np.abs(g_ref).max(), err_msg="%s d%s" % (tag, name))
        ref.step(want[3:])
        tabs = (("P", state.P, ref.params[0]), ("Q", state.Q, ref.params[1])) + ((("w", state.w, ref.params[2]),) if rubi else ())
        for name, mine, theirs in tabs:
            np.testing.assert_allclose(mine.cpu().numpy(), theirs, rtol=0, atol=2e-3 * LR * (t + 1), err_msg="%s %s step %d" % (tag, name, t))
    # (slots: the tolerance test_gpu_bpr.py / test_gpu_rubi_bpr.py grant these kinds against the same restatements)
    for name, mine, theirs in (("mP", state.mP, ref.m[0]), ("mQ", state.mQ, ref.m[1]), ("vP", state.vP, ref.v[0]), ("vQ", state.vQ, ref.v[1])):
        np.testing.assert_allclose(mine.cpu().numpy(), theirs, rtol=2e-4, atol=2e-6 * np.abs(theirs).max(), err_msg="%s %s" % (tag, name))
    assert_clean(state, tag)
    assert np.array_equal(state.wu.cpu().numpy(), wu), tag          # neither kind trains w_user
    if not rubi:
        assert np.array_equal(state.w.cpu().numpy(), w), tag
    res["losses"][tag] = got.tolist()


def lgcn_problem(d, B):
    """the problem of test_gpu_ops.py::test_lgcn_train_step_matches_oracle"""
    from test_gpu_ops import make_problem, toy_graph
    n_users, n_items, L = 500, 200, 2
    A = toy_graph(n_users, n_items, 5)
    P, Q, w, wu, u, i, j = make_problem(d, n_users, n_items, d, B)
    return n_users, n_items, L, A, np.concatenate([P, Q]).astype(np.float32), w, wu, u, i, j


def staging1_lgcn(ops, res, kind_name, d=64, B=256):
    """test_lgcn_train_step_matches_oracle at (d, B) = (64, 256), with its tolerances, the pair stage on the staged path"""
    kind, tag = getattr(oracle, kind_name), "lgcn %s B%d d%d" % (kind_name, B, d)
    n_users, n_items, L, A, T, w, wu, u, i, j = lgcn_problem(d, B)
    alpha, beta, decay, lr, bs = 1e-2, 1e-3, 1e-4, 1e-3, B
    st = oracle.AdamState([T.shape, (d,), (d,)])
    To, wo, wuo = T.copy(), w.copy(), wu.copy()
    state = ops.LGCNState(dev(T), n_users, n_items, dev(w), dev(wu), ops.CSR.from_scipy(A, "cuda"), L,
                          ops.make_hyper(lr, decay, alpha, beta, bs), B)
    rs = np.random.RandomState(2)
    for t in range(3):
        if t:
            u = rs.choice(n_users, B, replace=False).astype(np.int32)
            i = rs.randint(0, n_items, B).astype(np.int32)
            j = rs.randint(0, n_items, B).astype(np.int32)
        want = oracle.lgcn_train_step(kind, n_users, n_items, L, A.indptr, A.indices, A.data, u, i, j, To, wo, wuo, st, lr, decay,
                                      alpha, beta, bs)
        got, names = timed(ops, lambda: state.step(kind, dev(u), dev(i), dev(j)).cpu().numpy().copy())
        check_staged_names(names, (tag, t))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg="%s step %d" % (tag, t))
        if t == 0:
            res["names"][tag] = names
            g_hip, g_orc = state.mT.cpu().numpy() / 0.1, st.m[0] / 0.1
            np.testing.assert_allclose(g_hip, g_orc, rtol=5e-4, atol=2e-6 * np.abs(g_orc).max(), err_msg=tag)
        np.testing.assert_allclose(state.T.cpu().numpy(), To, rtol=0, atol=0.02 * lr * (t + 1), err_msg="%s step %d" % (tag, t))
    res["losses"][tag] = got.tolist()


def staging1(ops, res, part):
    for shape in STAGING_SHAPES:
        for kind_name in ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH", "LOSS_RUBIBCE"):
            staging1_bce(ops, res, kind_name, *shape)
        for kind_name in ("LOSS_BPR", "LOSS_RUBIBPR"):
            staging1_bpr(ops, res, kind_name, *shape)
    for kind_name in ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH"):
        staging1_lgcn(ops, res, kind_name)


# ----------------------------------------------------------------------------- MACR_EVAL_F32_SAMPLE
ALL_SCORE_KINDS = ("SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_RUBI", "SCORE_DIRECT_MINUS", "SCORE_DIRECT_MINUS_BOTH")
SWEEP_CS = (40.0, -2.5, 0.0)


def f32_ranking_case(ops, res, kind_name, d, K, want_f32_sample):
    """U = 300 queries against N = 5000 items at an item offset, random train lists and one query with 4 candidates, under the
    fp32 filter: the unseeded ranking, the seeded one after it and the sweep over three values of c equal oracle.score_topk
    bit for bit (ids, counts, score bits); the unseeded call's launch names say which sampling pass gave the thresholds."""
    import torch
    from macr_amd import _lib
    from test_gpu_ops import random_mask
    kind, tag = getattr(oracle, kind_name), "%s d%d K%d" % (kind_name, d, K)
    U, N, off = 300, 5000, 1000
    assert _lib.lib().macr_score_topk_uses_seeds(U, N, d) == 1, tag
    rs = np.random.RandomState(7000 + 17 * kind + d + K)
    P = (rs.standard_normal((U + 50, d)) * 0.4).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.4).astype(np.float32)
    uid = rs.permutation(U + 50)[:U].astype(np.int32)
    sig_u = (1.0 / (1.0 + np.exp(-rs.standard_normal(U) * 2.0))).astype(np.float32)
    sig_i = (1.0 / (1.0 + np.exp(-rs.standard_normal(N) * 2.0))).astype(np.float32)
    lists = [[x + off for x in row] for row in random_mask(rs, U, N, 30, heavy=(7,))]
    mcsr = oracle.csr_from_lists(lists)
    mask = ops.CSR(dev(mcsr[0]), dev(mcsr[1]))
    Pd, Qd, ud, sud, sid = dev(P), dev(Q), dev(uid), dev(sig_u), dev(sig_i)
    want = {}

    def oracle_lists(c):
        if c not in want:
            want[c] = oracle.score_topk(kind, P[uid], Q, K, sig_u, sig_i, c, mcsr, off)
        return want[c]

    def assert_is_oracle(vals, idx, c, what):
        gv, gi, gc = ops.topk_merge(vals.contiguous(), idx.contiguous())
        wv, wi, wc = oracle_lists(c)
        assert np.array_equal(gi.cpu().numpy(), wi), (tag, what, c)
        assert np.array_equal(gc.cpu().numpy(), wc), (tag, what, c)
        assert np.array_equal(gv.cpu().numpy().view(np.uint32), wv.view(np.uint32)), (tag, what, c)

    c = 0.0 if kind == oracle.SCORE_NORMAL else SWEEP_CS[0]
    seeds = torch.full((U, ops.SEED_WIDTH), -1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    names = {}
    for mode in ("unseeded", "seeded"):
        (v, ix), names[mode] = timed(ops, lambda: ops.score_topk(kind, Pd, ud, Qd, K, sud, sid, c, mask, off, filter="f32",
                                                                 seed=seeds if mode == "seeded" else None, seed_out=seeds, stats=stats))
        assert stats.cpu().numpy().tolist()[1] == 0, (tag, mode)         # the exact fallback kernel is not what ranks here
        assert_is_oracle(v, ix, c, mode)
    assert "tau_seed" in names["seeded"] and not {"score_sample", "score_sample_b"} & set(names["seeded"]), (tag, names["seeded"])
    if want_f32_sample:
        assert "score_sample" in names["unseeded"] and "score_sample_b" not in names["unseeded"], (tag, names["unseeded"])
    else:
        assert "score_sample_b" in names["unseeded"] and "score_sample" not in names["unseeded"], (tag, names["unseeded"])
    if kind != oracle.SCORE_NORMAL:                  # (a score without c has no sweep: macr_score_topk_sweep refuses it)
        cs = dev(np.asarray(SWEEP_CS, np.float32))
        (v, ix), names["sweep"] = timed(ops, lambda: ops.score_topk_sweep(kind, Pd, ud, Qd, K, sud, sid, cs, mask, off, filter="f32"))
        assert v.shape == (len(SWEEP_CS), U, K)
        for g, cg in enumerate(SWEEP_CS):
            assert_is_oracle(v[g:g + 1], ix[g:g + 1], cg, "sweep")
        # the sweep's fp32 filter has one sampling pass, the fp32 one, with or without the variable
        assert "score_sample" in names["sweep"] and "score_sample_b" not in names["sweep"], (tag, names["sweep"])
    res["names"][tag] = names


def f32_sample(ops, res, part):
    for kind_name in ALL_SCORE_KINDS:
        for d in (32, 64, 128, 256):
            for K in (5, 20):
                f32_ranking_case(ops, res, kind_name, d, K, True)


def f32_sample_off(ops, res, part):
    """the sibling: without the variable the unseeded fp32-filter ranking samples on the fp16 copies"""
    for kind_name, d, K in (("SCORE_NORMAL", 64, 20), ("SCORE_RUBI_BOTH", 128, 5), ("SCORE_DIRECT_MINUS_BOTH", 32, 20)):
        f32_ranking_case(ops, res, kind_name, d, K, False)


# ----------------------------------------------------------------------------- MACR_LGCN_DENSE=1
def lgcn_dense(ops, res, part):
    """With the variable every step keeps its layers dense, so the MACR_STEP_DENSE_LAYERS flag changes nothing: of two states,
    one stepped with dense_layers=True, both launch the kernels of the dense arm (separate regulariser and Adam launches, no
    fused finisher), the same ones in the same order, and the losses are the oracle's.  Identical BITS need a step whose
    result is a function of its inputs: this batch repeats rows (a hot positive item), and the plain step adds them with float
    atomics in order of arrival, so two runs of the same code differ in last bits.  The bit-for-bit half therefore runs on
    states with deterministic=True (MACR_STEP_DETERMINISTIC, which takes the flag too); the plain states are held to each other
    within the bounds of test_lgcn_batch_row_sparse_layers_equal_dense_layers."""
    d, B = 64, 256
    n_users, n_items, L, A, T, w, wu, u, i, j = lgcn_problem(d, B)
    alpha, beta, decay, lr, bs = 1e-2, 1e-3, 1e-4, 1e-3, B
    adj = ops.CSR.from_scipy(A, "cuda")
    for kind_name in ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH"):
        kind = getattr(oracle, kind_name)
        for det in (True, False):
            tag = "%s %s" % (kind_name, "deterministic" if det else "plain")
            st = oracle.AdamState([T.shape, (d,), (d,)])
            To, wo, wuo = T.copy(), w.copy(), wu.copy()
            states = [ops.LGCNState(dev(T), n_users, n_items, dev(w), dev(wu), adj, L, ops.make_hyper(lr, decay, alpha, beta, bs), B,
                                    deterministic=det) for _ in range(2)]
            rs = np.random.RandomState(2)
            bu, bi, bj = u, i, j
            for t in range(3):
                if t:
                    bu = rs.choice(n_users, B, replace=False).astype(np.int32)
                    bi = rs.randint(0, n_items, B).astype(np.int32)
                    bj = rs.randint(0, n_items, B).astype(np.int32)
                want = oracle.lgcn_train_step(kind, n_users, n_items, L, A.indptr, A.indices, A.data, bu, bi, bj, To, wo, wuo, st, lr,
                                              decay, alpha, beta, bs)
                out = [timed(ops, lambda s=s, flag=flag: s.step(kind, dev(bu), dev(bi), dev(bj), dense_layers=flag).cpu().numpy().copy())
                       for s, flag in zip(states, (False, True))]
                (la, na), (lb, nb) = out
                where = (tag, t)
                assert na == nb, (where, na, nb)                         # the same launches in the same order
                assert "adam_dense" in na and "lgcn_finalize" not in na and not any(n.endswith("+adam") for n in na), (where, na)
                assert ("reg_rows" if det else "reg_scatter") in na, (where, na)
                if det or t == 0:                                        # (the forward of equal tables is the same bits)
                    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (where, la, lb)
                np.testing.assert_allclose(la, lb, rtol=2e-6, err_msg=str(where))
                for name in ("T", "mT", "vT", "w", "wu", "adam_pow"):
                    a, b = getattr(states[0], name).cpu().numpy(), getattr(states[1], name).cpu().numpy()
                    if det:
                        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (where, name, int((a != b).sum()))
                    elif name in ("T", "w", "wu"):
                        np.testing.assert_allclose(a, b, rtol=0, atol=2e-3 * lr * (t + 1), err_msg="%s %s" % (where, name))
                for la_ in (la, lb):
                    np.testing.assert_allclose(la_, want, rtol=1e-5, atol=0, err_msg=str(where))
                for s in states:
                    np.testing.assert_allclose(s.T.cpu().numpy(), To, rtol=0, atol=0.02 * lr * (t + 1), err_msg=str(where))
            res["names"][tag] = na
            res["losses"][tag] = la.tolist()


SETTINGS = {"stage_listed0": stage_listed0, "staging1": staging1, "f32_sample": f32_sample, "f32_sample_off": f32_sample_off,
            "lgcn_dense": lgcn_dense}


def main(setting, part=None):
    env = {k: v for k, v in os.environ.items() if k.startswith("MACR_")}
    res = {"setting": setting, "part": part, "env": env, "names": {}, "losses": {}, "ok": False}
    if env != ENV[setting]:
        raise SystemExit("setting %s runs under %r, not under %r" % (setting, ENV[setting], env))
    from macr_amd import ops
    try:
        SETTINGS[setting](ops, res, part)
        res["ok"] = True
    except AssertionError:
        res["error"] = traceback.format_exc()[-3000:]
    res["names"] = {k: (sorted(set(v)) if isinstance(v, list) else {m: sorted(set(n)) for m, n in v.items()}) for k, v in res["names"].items()}
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
