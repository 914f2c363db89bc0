"""MF two-branch BPR loss (`--train rubi`, MACR_LOSS_RUBIBPR) without a GPU: the tests' float64 restatement
(tests/rubi_bpr_ref.py) matches the reference's own graph code (G13, tests/golden/make_golden_rubi_bpr.py); the ABI constant
agrees across the header, the ctypes bindings and ops; the model and the parser take the flag; the entry points take the
kind where they take RUBIBCE and refuse it where they refuse RUBIBCE_EGO."""
import os
import re

import numpy as np
import pytest

import rubi_bpr_ref
from helpers import GOLD, golden_npz_parts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("P", "Q", "w", "wu", "u", "i", "j")


def g13():
    with np.load(os.path.join(GOLD, "G13_mf_rubi_bpr.npz")) as z:
        return {k: z[k] for k in z.files}


def problem(tag, G=None):
    """the inputs of case `tag`: G10's arrays for a / b / c, G13's own for d"""
    if tag == "d":
        G = g13() if G is None else G
        return {k: G["mf_d/in/%s" % k] for k in INPUTS}
    G10 = golden_npz_parts("G10_model_steps")
    return {k: G10["mf_%s/%s" % (tag, k)] for k in INPUTS}


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_restated_rubi_bpr_matches_reference_graph(tag):
    G = g13()
    alpha, decay, bs = float(G["hyper"][0]), float(G["hyper"][2]), int(G["hyper"][3])
    g = problem(tag, G)
    loss, mf, reg, dP, dQ, dw = rubi_bpr_ref.mf_rubi_bpr(g["P"], g["Q"], g["w"], g["u"], g["i"], g["j"], alpha, decay, bs)
    w = lambda k: G["mf_%s/rubi_bpr/f64/%s" % (tag, k)]
    np.testing.assert_allclose([loss, mf, reg], [float(w("loss")), float(w("mf_loss")), float(w("reg_loss"))], rtol=1e-10)
    np.testing.assert_allclose(dP, w("dP"), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dQ, w("dQ"), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dw, w("dw").reshape(-1), rtol=1e-10, atol=1e-14)
    for k in ("loss", "mf_loss", "reg_loss"):                   # the fp32 graph is finite and agrees with the fp64 one on these cases
        np.testing.assert_allclose(float(G["mf_%s/rubi_bpr/f32/%s" % (tag, k)]), float(w(k)), rtol=1e-5)


def test_case_d_is_the_window_edge_case():
    """every cell of case d is finite in fp32 (Z > -88) while pairs of its cells are not under one shared logarithm
    (Z1 + Z2 < -88); case c stays inside"""
    for tag, lo, hi in (("c", -31.6, 48.2), ("d", -71.7, 57.7)):
        g = problem(tag)
        Z = rubi_bpr_ref.z_matrix(g["P"], g["Q"], g["w"], g["u"], g["i"], g["j"])
        np.testing.assert_allclose([Z.min(), Z.max()], [lo, hi], atol=0.06)
    assert -88.0 < Z.min() < -44.0


def test_overflow_problem_is_beyond_fp32():
    """the problem of the GPU overflow test: its smallest logit is below the fp32 range of log(sigmoid(Z)) (about -88)"""
    for k, v in zip(INPUTS, rubi_bpr_ref.mf_problem(14, 90, 50, 32, 96, 1.7)):      # the restated generator is the fixture's
        assert np.array_equal(v, g13()["mf_d/in/%s" % k]), k
    P, Q, w, wu, u, i, j = rubi_bpr_ref.mf_problem(14, 90, 50, 32, 96, 2.0)
    Z = rubi_bpr_ref.z_matrix(P, Q, w, u, i, j)
    np.testing.assert_allclose(Z.min(), -100.7, atol=0.06)


def test_restatement_on_torch_equals_the_numpy_form():
    """the (B,B) sums of the restatement in torch float64 (what the tests of the largest batches run on the device)"""
    P, Q, w, wu, u, i, j = rubi_bpr_ref.mf_problem(5, 300, 200, 32, 700, 0.8)
    a = rubi_bpr_ref.mf_rubi_bpr(P, Q, w, u, i, j, 1e-2, 1e-5, 1024)
    b = rubi_bpr_ref.mf_rubi_bpr(P, Q, w, u, i, j, 1e-2, 1e-5, 1024, device="cpu")
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-16)


def test_fixture_is_small_and_holds_outputs_only():
    path = os.path.join(GOLD, "G13_mf_rubi_bpr.npz")
    assert os.path.getsize(path) < 1 << 20
    assert all(k == "hyper" or "/rubi_bpr/" in k or k.startswith("mf_d/in/") for k in g13())


def test_loss_kind_constant_agrees_across_header_bindings_and_ops():
    from macr_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    consts = dict(re.findall(r"#define (MACR_LOSS_[A-Z_]+)\s+(\d+)", src))
    assert int(consts["MACR_LOSS_RUBIBPR"]) == _lib.LOSS_RUBIBPR == ops.LOSS_RUBIBPR == 6
    assert len(set(consts.values())) == len(consts) == 7
    assert int(re.search(r"#define MACR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 16
    assert not ops.is_pair_loss(ops.LOSS_RUBIBPR) and not _lib.is_pair_loss(6)


def test_model_and_parser_take_the_flag():
    import importlib.util
    from macr_amd import ops
    from macr_amd.mf import BPRMF, ShardedBPRMF
    assert BPRMF._TRAIN["rubi"][1] == ops.LOSS_RUBIBPR
    assert ops.LOSS_RUBIBPR in BPRMF._ON_DEMAND                 # table-sized optimizer state only once the loss trains
    assert BPRMF.kind_of(BPRMF.__new__(BPRMF), "rubi") == ops.LOSS_RUBIBPR
    with pytest.raises(NotImplementedError, match="row-sharded"):
        ShardedBPRMF.kind_of(ShardedBPRMF.__new__(ShardedBPRMF), "rubi")
    with pytest.raises(NotImplementedError, match="rubi \\| rubibce"):
        BPRMF.kind_of(BPRMF.__new__(BPRMF), "userc")
    spec = importlib.util.spec_from_file_location("macr_mf_parse", os.path.join(REPO, "macr_mf", "parse.py"))
    parse = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parse)
    assert parse.parse_args(["--train", "rubi", "--test", "rubi"]).train == "rubi"
    assert "rubi (two-branch BPR)" in parse.build_parser().format_help()


def test_entry_points_take_the_kind_where_they_take_rubibce():
    """Argument validation comes before any device work, so this needs no GPU (the pointers are never dereferenced): the MF
    step, its lazy form and both flushes answer kind 6 as they answer RUBIBCE -- the step gets as far as the workspace check
    -- every shard entry point answers it as it answers RUBIBCE_EGO, and the LightGCN step refuses it."""
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
    mf_calls = {
        "step": lambda k, ws: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, 0, p, ws, None),
        "step_deferred": lambda k, ws: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p,
                                                            _lib.STEP_DEFER, p, ws, None),
        "step_pending": lambda k, ws: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p,
                                                           _lib.STEP_DEFER | _lib.STEP_PENDING, p, ws, None),
        "step_lazy": lambda k, ws: L.macr_mf_train_step_lazy(k, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p,
                                                             _lib.STEP_DEFER, ctypes.byref(lz), p, ws, None),
        "flush": lambda k, ws: L.macr_mf_train_flush(k, B, d, 100, 100, *([p] * 16), ctypes.byref(hp), p, ws, None),
        "flush_lazy": lambda k, ws: L.macr_mf_train_flush_lazy(k, B, d, 100, 100, *([p] * 16), ctypes.byref(hp), ctypes.byref(lz),
                                                               p, ws, None),
    }
    for name, call in mf_calls.items():                          # a workspace of 16 bytes: the last check before any launch
        rc = call(_lib.LOSS_RUBIBCE, 16)
        assert rc == _lib.E_WORKSPACE, (name, rc)
        assert call(_lib.LOSS_RUBIBPR, 16) == rc, (name, L.macr_last_error())
        assert b"workspace" in L.macr_last_error(), name
    # the step without its branch vector is refused like RUBIBCE's
    no_w = lambda k: L.macr_mf_train_step(k, B, d, 100, 100, p, p, p, p, p, None, p, *([p] * 12), p, ctypes.byref(hp), p, 0, p,
                                          1 << 30, None)
    assert no_w(_lib.LOSS_RUBIBPR) == no_w(_lib.LOSS_RUBIBCE) == _lib.E_INVALID
    shard_calls = {
        "forward": lambda k: L.macr_shard_forward(k, B, d, p, p, p, p, 1 << 30, None),
        "forward_slice": lambda k: L.macr_shard_forward_slice(k, B, d, 0, B, p, p, p, p, p, p, 1 << 30, None),
        "backward_slice": lambda k: L.macr_shard_backward_slice(k, B, d, 0, B, p, p, p, p, ctypes.byref(hp), p, p, p, p, p,
                                                                1 << 30, None),
    }
    for name, call in shard_calls.items():
        rc = call(_lib.LOSS_RUBIBCE_EGO)
        assert rc in (_lib.E_INVALID, _lib.E_UNSUPPORTED), (name, rc)
        assert call(_lib.LOSS_RUBIBPR) == rc, name
    assert L.macr_lgcn_train_step(_lib.LOSS_RUBIBPR, B, d, 50, 50, 2, p, p, p, None, None, p, p, p, *([p] * 9), p, ctypes.byref(hp),
                                  p, 0, p, 1 << 30, None) == _lib.E_INVALID
    assert b"loss_kind=6" in L.macr_last_error()
