"""LightGCN's `--loss bce` / `--loss bceboth` without a GPU: the tests' float64 restatement (tests/lgcn_both_ref.py) matches
the reference's own graph code (G10, tests/golden/make_golden_model.py), and the fp32 C oracle, run beside it for the twenty
steps of tests/test_gpu_lgcn_trajectory.py at 0 to 5 layers, stays within a TENTH of every tolerance that test holds the HIP
step to -- so a HIP step that misses one of them is further from the float64 truth than plain fp32 arithmetic explains."""
import numpy as np
import pytest
import scipy.sparse as sp

import lgcn_both_ref as lb
import oracle
from helpers import golden_npz_parts


@pytest.mark.parametrize("loss", ["bce", "bceboth"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_losses_match_reference_graph(tag, loss):
    G10 = golden_npz_parts("G10_model_steps")
    alpha, beta, decay, bs = float(G10["hyper"][0]), float(G10["hyper"][1]), float(G10["hyper"][2]), int(G10["hyper"][3])
    g = lambda k: G10["lgcn_%s/%s" % (tag, k)]
    P, Q = g("P"), g("Q")
    A = sp.csr_matrix((g("data"), g("indices"), g("indptr")), shape=(P.shape[0] + Q.shape[0],) * 2).astype(np.float64)
    got = lb.lgcn_both(A, np.concatenate([P, Q]), g("w"), g("wu"), P.shape[0], 2, g("u"), g("i"), g("j"), alpha, beta, decay, bs,
                       both=loss == "bceboth")
    want = lambda k: np.asarray(g("%s/f64/%s" % (loss, k)), np.float64)
    np.testing.assert_allclose(got[:3], [float(want("loss")), float(want("mf_loss")), float(want("emb_loss"))], rtol=1e-12)
    dT = np.concatenate([want("dP"), want("dQ")])
    for name, x, y in (("dT", got[3], dT), ("dw", got[4], want("dw").reshape(-1)), ("dwu", got[5], want("dwu").reshape(-1))):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12 * np.abs(y).max(), err_msg=name)
    if loss == "bce":
        assert not want("dw").any() and not want("dwu").any() and not got[4].any() and not got[5].any()
    else:
        assert want("dw").any() and want("dwu").any()


@pytest.mark.parametrize("kind", ["bce", "bceboth"])
@pytest.mark.parametrize("asym", [False, True], ids=["sym", "rownorm"])
@pytest.mark.parametrize("d", [32, 256])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 4, 5])
def test_fp32_oracle_uses_a_tenth_of_the_trajectory_tolerances(L, d, asym, kind, record_property):
    B = 512
    pr, ref = lb.problem(asym, L, d, B), lb.reference(kind, asym, L, d, B)
    A, At = pr["A"], pr["At"]
    T, w, wu = pr["T"].copy(), pr["w"].copy(), pr["wu"].copy()
    st = oracle.AdamState([T.shape, (d,), (d,)])
    okind = oracle.LOSS_RUBIBCEBOTH if kind == "bceboth" else oracle.LOSS_NORMALBCE
    tr = None if At is None else (At.indptr, At.indices, At.data)
    ratios = {"losses": 0.0}
    for t, (u, i, j) in enumerate(pr["batches"][:lb.STEPS]):
        got = oracle.lgcn_train_step(okind, lb.N_USERS, lb.N_ITEMS, L, A.indptr, A.indices, A.data, u, i, j, T, w, wu, st,
                                     lb.LR, lb.DECAY, lb.ALPHA, lb.BETA, lb.BS, transposed=tr)
        rel = np.abs(np.asarray(got, np.float64) - ref["losses"][t]) / np.abs(ref["losses"][t])
        ratios["losses"] = max(ratios["losses"], float(rel.max() / 1e-5))
    state = dict(T=T, w=w, wu=wu, mT=st.m[0], vT=st.v[0], mw=st.m[1], vw=st.v[1], mwu=st.m[2], vwu=st.v[2])
    for name in ("T", "w", "wu") + lb.SLOTS:
        ratios.update(lb.used(state[name], ref[name], name))
    want_pow = np.array([0.9, 0.999]) * np.array([0.9 ** lb.STEPS, 0.999 ** lb.STEPS])     # (on entry: the first step's powers)
    ratios["adam_pow"] = float((np.abs(st.power - want_pow) / want_pow).max() / 1e-6)
    for k, v in sorted(ratios.items()):
        record_property(k, v)
    print("L=%d d=%d %s %s: share of the GPU tolerances the fp32 oracle uses: %s" % (
        L, d, "rownorm" if asym else "sym", kind, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    # A tenth: of the loss tolerance, of both bounds on T, w, wu, and of the slots' RELATIVE tolerance once their absolute part
    # (2e-6 max |want|) is granted -- "<slot> rtol".  The absolute part is not divisible: fp32 rounding of the gradient's
    # largest terms lands on its small elements at that scale, so the plain ratio diff / bound of a slot ("<slot>", up to
    # 0.53 for mT, 0.35 for mw) is held below 1 only.  adam_pow is twenty products by fp32(0.9), which is 2.6e-8 off 0.9:
    # 0.55 of its 1e-6 whatever computes it in fp32.
    tenth = {k: v for k, v in ratios.items() if k not in lb.SLOTS + ("adam_pow",)}
    assert max(tenth.values()) <= 0.1, tenth
    assert max(ratios.values()) <= 1.0, ratios
    if kind == "bce":                                    # the oracle, too, leaves the branch vectors and their slots alone
        assert np.array_equal(w, pr["w"]) and np.array_equal(wu, pr["wu"])
        assert not any(state[n].any() for n in ("mw", "vw", "mwu", "vwu"))
