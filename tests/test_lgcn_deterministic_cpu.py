"""The bit-reproducible LightGCN step (MACR_STEP_DETERMINISTIC on macr_lgcn_train_step / _t, include/macr_hip.h) without a GPU:
what the entry points accept and refuse, the size functions, the model's switch and the parser.  Argument validation comes
before any device work, so the pointers handed in are never dereferenced (as in tests/test_deterministic_cpu.py)."""
import ctypes
import importlib.util
import os
import re
import types

import pytest

from helpers import REPO, golden

DET, LOSS_ONLY, DENSE = 16, 4, 8
KINDS = ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH", "LOSS_BPR_LGCN", "LOSS_RUBIBCE", "LOSS_RUBIBCE_EGO")
N_USERS, N_ITEMS = 100, 100


@pytest.fixture(scope="module")
def L():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib.lib()


def _plan_header(N, n_slots=3, n_groups=2, n_split=1):
    """the eight int32 a plan starts with (spmm_kernels.hip PlanHeader): all the size functions read"""
    return (ctypes.c_int32 * 16)(0x4d414356, N, n_split, n_slots, N, 64, n_groups, 0)


def _step(L, kind, flags, ws_bytes=1 << 40, B=64, d=64, transposed=False):
    from macr_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    hp = _lib.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-5, 1e-2, 1e-3, 1024)
    head = [kind, B, d, N_USERS, N_ITEMS, 2, p, p, p, None, None]
    tail = [p, p, p] + [p] * 10 + [ctypes.byref(hp), p, flags, p, ws_bytes, None]
    if transposed:
        return L.macr_lgcn_train_step_t(*(head + [p, p, p, None, None] + tail))
    return L.macr_lgcn_train_step(*(head + tail))


def test_flag_and_abi_version():
    from macr_amd import _lib
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    assert int(re.search(r"#define MACR_STEP_DETERMINISTIC\s+(\d+)", src).group(1)) == _lib.STEP_DETERMINISTIC == DET
    assert int(re.search(r"#define MACR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 16     # additive: the ABI stays
    assert (_lib.STEP_LOSS_ONLY, _lib.STEP_DENSE_LAYERS) == (LOSS_ONLY, DENSE)
    for name in ("macr_lgcn_train_workspace_bytes_det", "macr_lgcn_train_workspace_bytes_det_t"):
        assert name in _lib.SIGNATURES and re.search(r"size_t %s\(" % name, src), name


@pytest.mark.parametrize("transposed", [False, True])
def test_steps_know_the_flag_and_ask_for_the_workspace(L, transposed):
    from macr_amd import _lib
    for kind in KINDS:
        for flags in (DET, DET | LOSS_ONLY, DET | DENSE, DET | LOSS_ONLY | DENSE):
            rc = _step(L, getattr(_lib, kind), flags, ws_bytes=16, transposed=transposed)
            assert rc == _lib.E_WORKSPACE, (kind, flags, rc, L.macr_last_error())
            assert b"workspace" in L.macr_last_error()


@pytest.mark.parametrize("transposed", [False, True])
def test_unknown_flag_bits_are_invalid(L, transposed):
    from macr_amd import _lib
    for flags in (32, 32 | DET, 1, 2 | DET):
        assert _step(L, _lib.LOSS_RUBIBCEBOTH, flags, transposed=transposed) == _lib.E_INVALID, flags
        assert ("flags=%d" % flags).encode() in L.macr_last_error()


def test_size_functions(L):
    N = N_USERS + N_ITEMS
    plan, plan_t = _plan_header(N), _plan_header(N, n_slots=7, n_groups=3, n_split=2)
    for ph, pt in ((None, None), (plan, plan_t)):
        for B in (1, 96, 257, 300, 4096, 8448, 65536):
            for d in (32, 64, 128, 256):
                plain, det = L.macr_lgcn_train_workspace_bytes(B, N, d, ph), L.macr_lgcn_train_workspace_bytes_det(B, N, d, ph)
                assert det >= plain > 0, (B, d, plain, det)
                plain_t = L.macr_lgcn_train_workspace_bytes_t(B, N, d, ph, pt)
                det_t = L.macr_lgcn_train_workspace_bytes_det_t(B, N, d, ph, pt)
                assert det_t >= plain_t > 0 and det_t >= det, (B, d, plain_t, det_t)
        for B, d in ((300, 48), (0, 64)):
            assert L.macr_lgcn_train_workspace_bytes(B, N, d, ph) == 0
            assert L.macr_lgcn_train_workspace_bytes_det(B, N, d, ph) == 0
            assert L.macr_lgcn_train_workspace_bytes_det_t(B, N, d, ph, pt) == 0
        assert L.macr_lgcn_train_workspace_bytes_det(64, 0, 64, ph) == 0


@pytest.mark.parametrize("transposed", [False, True])
def test_the_plain_size_is_not_enough_for_the_flag(L, transposed):
    from macr_amd import _lib
    N = N_USERS + N_ITEMS
    plain, det = L.macr_lgcn_train_workspace_bytes(64, N, 64, None), L.macr_lgcn_train_workspace_bytes_det(64, N, 64, None)
    assert det > plain
    for kind in KINDS:
        assert _step(L, getattr(_lib, kind), DET, ws_bytes=plain, transposed=transposed) == _lib.E_WORKSPACE, kind
        assert _step(L, getattr(_lib, kind), DET, ws_bytes=det - 1, transposed=transposed) == _lib.E_WORKSPACE, kind


def test_lightgcn_reads_the_variable(monkeypatch):
    """the switch is taken before anything touches a device: stop the constructor right behind it"""
    from macr_amd.lightgcn import LightGCN

    class Stop(Exception):
        pass

    class Args(types.SimpleNamespace):
        @property
        def adj_type(self):                      # the first thing the constructor reads after the switch and its refusals
            raise Stop()

    def switch(**kw):
        m = LightGCN.__new__(LightGCN)
        with pytest.raises(Stop):
            m.__init__(dict(n_users=3, n_items=2, norm_adj=None), Args(alg_type="lightgcn", node_dropout_flag=0), **kw)
        return m.deterministic

    monkeypatch.delenv("MACR_DETERMINISTIC", raising=False)
    assert switch() is False and switch(deterministic=True) is True
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")
    assert switch() is True and switch(deterministic=False) is False
    monkeypatch.setenv("MACR_DETERMINISTIC", "0")
    assert switch() is False


def test_lgcn_state_takes_the_keyword():
    import inspect
    from macr_amd import ops
    from macr_amd.lightgcn import LightGCN
    assert inspect.signature(ops.LGCNState.__init__).parameters["deterministic"].default is False
    assert inspect.signature(LightGCN.__init__).parameters["deterministic"].default is None


def test_lightgcn_parser_gains_no_flag():
    spec = importlib.util.spec_from_file_location("lg_parser_det", os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ours = vars(mod.parse_args([]))
    assert set(ours) - set(golden("lgcn", "tiny")["G9"]) == {"seed", "sampler", "resume"}
