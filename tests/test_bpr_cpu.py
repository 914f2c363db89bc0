"""BPR losses (MF `--train normal`, LightGCN `--loss bpr`) without a GPU: the ABI constants agree across the header, the ctypes
bindings and ops; the models map the reference's flags to them; the tests' float64 restatement (tests/bpr_ref.py) matches
the reference's own graph code (G11, tests/golden/make_golden_bpr.py)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bpr_ref
from helpers import GOLD, golden_npz_parts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g11():
    with np.load(os.path.join(GOLD, "G11_bpr_steps.npz")) as z:
        return {k: z[k] for k in z.files}


def test_loss_kind_constants_agree_across_header_bindings_and_ops():
    from macr_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    consts = dict(re.findall(r"#define (MACR_LOSS_[A-Z_]+)\s+(\d+)", src))
    assert int(consts["MACR_LOSS_BPR"]) == _lib.LOSS_BPR == ops.LOSS_BPR == 3
    assert int(consts["MACR_LOSS_BPR_LGCN"]) == _lib.LOSS_BPR_LGCN == ops.LOSS_BPR_LGCN == 4
    assert int(re.search(r"#define MACR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 16
    assert [k for k in range(5) if ops.is_pair_loss(k)] == [ops.LOSS_NORMALBCE, ops.LOSS_BPR, ops.LOSS_BPR_LGCN]


def test_models_map_the_reference_flags_to_the_bpr_kinds():
    from macr_amd import ops
    from macr_amd.lightgcn import LightGCN
    from macr_amd.mf import BPRMF, ShardedBPRMF
    assert BPRMF._TRAIN["normal"][1] == ops.LOSS_BPR and ShardedBPRMF._TRAIN["normal"][1] == ops.LOSS_BPR
    assert LightGCN._LOSS["bpr"][1] == ops.LOSS_BPR_LGCN
    assert ops.LOSS_BPR in BPRMF._ON_DEMAND and ops.LOSS_BPR_LGCN in LightGCN._ON_DEMAND
    # the parser default of the LightGCN CLI is a loss the model serves
    from macr_lightgcn.utility import parser
    assert parser.parse_args([]).loss in LightGCN._LOSS


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restated_mf_bpr_matches_reference_graph(tag):
    G10, G = golden_npz_parts("G10_model_steps"), g11()
    decay, bs = float(G["hyper"][2]), int(G["hyper"][3])
    g = lambda k: G10["mf_%s/%s" % (tag, k)]
    loss, mf, reg, dP, dQ = bpr_ref.mf_bpr(g("P"), g("Q"), g("u"), g("i"), g("j"), decay, bs)
    w = lambda k: G["mf_%s/bpr/f64/%s" % (tag, k)]
    np.testing.assert_allclose([loss, mf, reg], [float(w("loss")), float(w("mf_loss")), float(w("reg_loss"))], rtol=1e-10)
    np.testing.assert_allclose(dP, w("dP"), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dQ, w("dQ"), rtol=1e-10, atol=1e-14)
    assert not w("dw").any() and not w("dwu").any()            # `opt` trains the `parameter` scope only (:52-57)
    for k in ("loss", "mf_loss", "reg_loss"):                   # the fp32 graph agrees with the fp64 one on these cases
        np.testing.assert_allclose(float(G["mf_%s/bpr/f32/%s" % (tag, k)]), float(w(k)), rtol=1e-5)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_lightgcn_bpr_matches_reference_graph(tag):
    G10, G = golden_npz_parts("G10_model_steps"), g11()
    decay, bs = float(G["hyper"][2]), int(G["hyper"][3])
    g = lambda k: G10["lgcn_%s/%s" % (tag, k)]
    P, Q = g("P"), g("Q")
    N = P.shape[0] + Q.shape[0]
    A = sp.csr_matrix((g("data").astype(np.float64), g("indices"), g("indptr")), shape=(N, N))
    loss, mf, emb, dT = bpr_ref.lgcn_bpr(A, np.concatenate([P, Q]), P.shape[0], 2, g("u"), g("i"), g("j"), decay, bs)
    w = lambda k: G["lgcn_%s/bpr/f64/%s" % (tag, k)]
    np.testing.assert_allclose([loss, mf, emb], [float(w("loss")), float(w("mf_loss")), float(w("emb_loss"))], rtol=1e-10)
    # (G10's adjacency is stored in fp32, as the reference builds it; the graph propagates in its own dtype)
    np.testing.assert_allclose(dT, np.concatenate([w("dP"), w("dQ")]), rtol=1e-10, atol=1e-14)
    assert not w("dw").any() and not w("dwu").any()


def test_restated_adam_is_the_oracle_rule():
    rs = np.random.RandomState(0)
    th = rs.standard_normal(50)
    opt = bpr_ref.Adam([th], 1e-3)
    gs = [rs.standard_normal(50) * 10.0 ** -k for k in range(1, 6)]
    m, v, t = np.zeros(50), np.zeros(50), th.copy()
    for k, gr in enumerate(gs, 1):
        opt.step([gr])
        m = 0.9 * m + 0.1 * gr
        v = 0.999 * v + 0.001 * gr * gr
        t = t - 1e-3 * np.sqrt(1 - 0.999 ** k) / (1 - 0.9 ** k) * m / (np.sqrt(v) + 1e-8)
    np.testing.assert_allclose(opt.params[0], t, rtol=1e-14)


def test_fixture_is_small_and_holds_outputs_only():
    path = os.path.join(GOLD, "G11_bpr_steps.npz")
    assert os.path.getsize(path) < 1 << 20
    keys = g11().keys()
    assert all(k == "hyper" or "/bpr/" in k for k in keys)


def test_entry_points_refuse_the_bpr_kinds_as_they_refuse_normalbce():
    """The rule of include/macr_hip.h: where NORMALBCE is refused (deferred mode, the lazy step, the flushes, the split step)
    the per-pair kinds are refused with the same code; a kind of the other model is an invalid argument.  Argument
    validation comes before any device work, so this needs no GPU (the pointers are never dereferenced)."""
    import ctypes
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    hp = _lib.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-5, 1e-2, 1e-3, 1024)
    lz = _lib.LazyAdam(p, p, p, 4)
    B, d = 64, 64
    calls = {
        "step_deferred": lambda k: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p,
                                                        _lib.STEP_DEFER, p, 1 << 30, None),
        "step_lazy": lambda k: L.macr_mf_train_step_lazy(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, 0,
                                                         ctypes.byref(lz), p, 1 << 30, None),
        "flush": lambda k: L.macr_mf_train_flush(k, B, d, 100, 100, *([p] * 16), ctypes.byref(hp), p, 1 << 30, None),
        "flush_lazy": lambda k: L.macr_mf_train_flush_lazy(k, B, d, 100, 100, *([p] * 16), ctypes.byref(hp), ctypes.byref(lz),
                                                           p, 1 << 30, None),
        "forward_slice": lambda k: L.macr_shard_forward_slice(k, B, d, 0, B, p, p, p, p, p, p, 1 << 30, None),
        "backward_slice": lambda k: L.macr_shard_backward_slice(k, B, d, 0, B, p, p, p, p, ctypes.byref(hp), p, p, p, p, p,
                                                                1 << 30, None),
    }
    for name, call in calls.items():
        rc = call(_lib.LOSS_NORMALBCE)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED), (name, rc)
        assert call(_lib.LOSS_BPR) == rc, name
        assert call(_lib.LOSS_BPR_LGCN) == rc or name.startswith("step"), name
    # each BPR kind belongs to one model
    assert L.macr_mf_train_step(_lib.LOSS_BPR_LGCN, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, 0, p, 1 << 30,
                                None) == _lib.E_INVALID
    assert b"loss_kind=4" in L.macr_last_error()
    assert L.macr_shard_forward(_lib.LOSS_BPR_LGCN, B, d, p, p, p, p, 1 << 30, None) == _lib.E_INVALID
    assert L.macr_lgcn_train_step(_lib.LOSS_BPR, B, d, 50, 50, 2, p, p, p, None, None, p, p, p, *([p] * 9), p, ctypes.byref(hp),
                                  p, 0, p, 1 << 30, None) == _lib.E_INVALID
    assert b"loss_kind=3" in L.macr_last_error()
