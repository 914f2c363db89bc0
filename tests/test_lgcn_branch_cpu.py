"""LightGCN's item-branch losses (`--loss bce1` / `bce2`) and rankings (`--test rubi1` / `rubi2`) without a GPU: the new loss kind
agrees across the header, the ctypes bindings and ops; the models and the CLI map the reference's flags to it; the entry
points validate it; the tests' float64 restatement (tests/lgcn_branch_ref.py) matches the reference's own graph code (G12,
tests/golden/make_golden_lgcn_branch.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bpr_ref
import lgcn_branch_ref
from helpers import GOLD, golden_npz_parts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g12():
    with np.load(os.path.join(GOLD, "G12_lgcn_item_branch.npz")) as z:
        return {k: z[k] for k in z.files}


def case(tag):
    G10 = golden_npz_parts("G10_model_steps")
    g = lambda k: G10["lgcn_%s/%s" % (tag, k)]
    P, Q = g("P"), g("Q")
    A = sp.csr_matrix((g("data"), g("indices"), g("indptr")), shape=(P.shape[0] + Q.shape[0],) * 2).astype(np.float64)
    return A, P, Q, g("w").reshape(-1), g("wu").reshape(-1), g("u"), g("i"), g("j")


def test_loss_kind_constant_agrees_across_header_bindings_and_ops():
    from macr_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    consts = dict(re.findall(r"#define (MACR_LOSS_[A-Z_]+)\s+(\d+)", src))
    assert int(consts["MACR_LOSS_RUBIBCE_EGO"]) == _lib.LOSS_RUBIBCE_EGO == ops.LOSS_RUBIBCE_EGO == 5
    assert int(re.search(r"#define MACR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 16
    assert not ops.is_pair_loss(ops.LOSS_RUBIBCE_EGO) and not ops.is_pair_loss(ops.LOSS_RUBIBCE)
    assert "macr_score_topk_prologue_prep_branch" in src and "macr_score_topk_prologue_prep_branch" in _lib.SIGNATURES


def test_models_and_cli_map_the_reference_flags():
    from macr_amd import ops
    from macr_amd.lightgcn import LightGCN
    assert LightGCN._LOSS["bce1"] == ("two_bce1", ops.LOSS_RUBIBCE)
    assert LightGCN._LOSS["bce2"] == ("two_bce2", ops.LOSS_RUBIBCE_EGO)
    assert ops.LOSS_RUBIBCE in LightGCN._ON_DEMAND and ops.LOSS_RUBIBCE_EGO in LightGCN._ON_DEMAND
    from macr_lightgcn.utility import parser
    a = parser.parse_args(["--loss", "bce2", "--test", "rubi2"])
    assert (a.loss, a.test) == ("bce2", "rubi2")
    assert parser.parse_args(["--loss", "bce1", "--test", "rubi1"]).loss in LightGCN._LOSS


def test_entry_points_validate_the_ego_kind():
    """MF and row-sharded entry points refuse RUBIBCE_EGO with the code they return for BPR_LGCN; the LightGCN step takes
    RUBIBCE and RUBIBCE_EGO (it gets as far as the workspace check).  Argument validation comes before any device work."""
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
        "step": lambda k: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, 0, p, 1 << 30, None),
        "step_lazy": lambda k: L.macr_mf_train_step_lazy(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, 0,
                                                         ctypes.byref(lz), p, 1 << 30, None),
        "flush": lambda k: L.macr_mf_train_flush(k, B, d, 100, 100, *([p] * 16), ctypes.byref(hp), p, 1 << 30, None),
        "shard_forward": lambda k: L.macr_shard_forward(k, B, d, p, p, p, p, 1 << 30, None),
        "forward_slice": lambda k: L.macr_shard_forward_slice(k, B, d, 0, B, p, p, p, p, p, p, 1 << 30, None),
        "backward_slice": lambda k: L.macr_shard_backward_slice(k, B, d, 0, B, p, p, p, p, ctypes.byref(hp), p, p, p, p, p,
                                                                1 << 30, None),
    }
    for name, call in calls.items():
        rc = call(_lib.LOSS_BPR_LGCN)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED), (name, rc)
        assert call(_lib.LOSS_RUBIBCE_EGO) == rc, name
    lgcn = lambda k: L.macr_lgcn_train_step(k, B, d, 50, 50, 2, p, p, p, None, None, p, p, p, *([p] * 9), p, ctypes.byref(hp),
                                            p, 0, p, 0, None)
    for k in (_lib.LOSS_RUBIBCE, _lib.LOSS_RUBIBCE_EGO, _lib.LOSS_RUBIBCEBOTH):
        assert lgcn(k) == _lib.E_WORKSPACE, (k, L.macr_last_error())
    assert lgcn(_lib.LOSS_BPR) == _lib.E_INVALID and lgcn(6) == _lib.E_INVALID


@pytest.mark.parametrize("loss", ["bce1", "bce2"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_item_branch_losses_match_reference_graph(tag, loss):
    A, P, Q, w, wu, u, i, j = case(tag)
    G = g12()
    alpha, decay, bs = float(G["hyper"][0]), float(G["hyper"][2]), int(G["hyper"][3])
    T = np.concatenate([P, Q]).astype(np.float64)
    got = lgcn_branch_ref.lgcn_item_branch(A, T, w, P.shape[0], 2, u, i, j, alpha, decay, bs, ego=loss == "bce2")
    want = lambda k: G["lgcn_%s/%s/f64/%s" % (tag, loss, k)]
    np.testing.assert_allclose(got[:3], [float(want("loss")), float(want("mf_loss")), float(want("emb_loss"))], rtol=1e-10)
    np.testing.assert_allclose(got[3], np.concatenate([want("dP"), want("dQ")]), rtol=1e-8, atol=1e-14)
    np.testing.assert_allclose(got[4], want("dw").reshape(-1), rtol=1e-8, atol=1e-14)
    assert not want("dwu").any() and float(want("reg_loss")) == 0.0       # w_user untouched; reg_loss is tf.constant(0.)
    for k in ("loss", "mf_loss", "emb_loss"):
        np.testing.assert_allclose(float(G["lgcn_%s/%s/f32/%s" % (tag, loss, k)]), float(want(k)), rtol=1e-5)


@pytest.mark.parametrize("loss", ["bce1", "bce2"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restated_rubi_rankings_match_reference_graph(tag, loss):
    """rubi_ratings1 / rubi_ratings2: (y_ui - c) sig(e_i . w), the branch on the propagated / the ego item rows"""
    A, P, Q, w, wu, u, i, j = case(tag)
    G = g12()
    c = float(G["hyper"][4])
    T = np.concatenate([P, Q]).astype(np.float64)
    nu = P.shape[0]
    E = bpr_ref.propagate(A, T, 2)
    sig = lgcn_branch_ref.rubi_sig(A, T, w, nu, 2, ego=loss == "bce2")
    want = (E[u] @ E[nu + i].T - c) * sig[i][None, :]
    np.testing.assert_allclose(want, G["lgcn_%s/%s/f64/ratings" % (tag, loss)], rtol=1e-9, atol=1e-12)


def test_fixture_is_small_and_holds_outputs_only():
    path = os.path.join(GOLD, "G12_lgcn_item_branch.npz")
    assert os.path.getsize(path) < 1 << 20
    G = g12()
    assert not any(k.endswith(("/P", "/Q", "/w", "/u", "/i", "/j")) for k in G)
