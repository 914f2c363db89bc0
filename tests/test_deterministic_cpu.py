"""The bit-reproducible MF step (MACR_STEP_DETERMINISTIC, include/macr_hip.h) without a GPU: the constant across the header, the
ctypes bindings and ops; the size function; what the entry points refuse.  Argument validation comes before any device work, so
the pointers handed in are never dereferenced (as in tests/test_bpr_cpu.py)."""
import ctypes
import importlib.util
import os
import re
import types

import pytest

from helpers import REPO, golden


@pytest.fixture(scope="module")
def L():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib.lib()


def _step_args():
    from macr_amd import _lib
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    hp = _lib.Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-5, 1e-2, 1e-3, 1024)
    return buf, p, hp


def _step(L, kind, flags, ws_bytes=1 << 30, B=64, d=64):
    buf, p, hp = _step_args()
    return L.macr_mf_train_step(kind, B, d, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, flags, p, ws_bytes, None)


def test_flag_agrees_across_header_bindings_and_ops():
    from macr_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    assert int(re.search(r"#define MACR_STEP_DETERMINISTIC\s+(\d+)", src).group(1)) == _lib.STEP_DETERMINISTIC == ops.STEP_DETERMINISTIC == 16
    assert int(re.search(r"#define MACR_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ABI_VERSION == 16     # additive: the ABI stays
    others = (_lib.STEP_DEFER, _lib.STEP_PENDING, _lib.STEP_LOSS_ONLY, _lib.STEP_DENSE_LAYERS)
    assert all(_lib.STEP_DETERMINISTIC & f == 0 for f in others)


def test_workspace_size_function(L):
    assert L.macr_mf_train_workspace_bytes_det(4096, 64) >= L.macr_mf_train_workspace_bytes(4096, 64) > 0
    assert L.macr_mf_train_workspace_bytes_det(4096, 48) == 0
    assert L.macr_mf_train_workspace_bytes_det(0, 64) == 0
    for B in (1, 96, 257, 300, 4096, 8192, 8448, 65536, 1 << 20):       # both sides of the default path's staging threshold
        for d in (32, 64, 128, 256):
            assert L.macr_mf_train_workspace_bytes_det(B, d) >= L.macr_mf_train_workspace_bytes(B, d) > 0, (B, d)


def test_step_refuses_a_small_workspace_with_the_flag(L):
    from macr_amd import _lib
    for kind in (_lib.LOSS_NORMALBCE, _lib.LOSS_RUBIBCEBOTH, _lib.LOSS_RUBIBCE, _lib.LOSS_BPR, _lib.LOSS_RUBIBPR):
        assert _step(L, kind, _lib.STEP_DETERMINISTIC, ws_bytes=16) == _lib.E_WORKSPACE, kind
        assert b"workspace" in L.macr_last_error()
    # the plain size is not enough for the deterministic step at a batch of the small-batch path
    plain, det = L.macr_mf_train_workspace_bytes(64, 64), L.macr_mf_train_workspace_bytes_det(64, 64)
    assert det > plain
    assert _step(L, _lib.LOSS_RUBIBCEBOTH, _lib.STEP_DETERMINISTIC, ws_bytes=plain) == _lib.E_WORKSPACE


def test_lazy_step_refuses_the_flag(L):
    from macr_amd import _lib
    buf, p, hp = _step_args()
    lz = _lib.LazyAdam(p, p, p, 4)
    for flags in (_lib.STEP_DETERMINISTIC, _lib.STEP_DETERMINISTIC | _lib.STEP_DEFER):
        rc = L.macr_mf_train_step_lazy(_lib.LOSS_RUBIBCEBOTH, 64, 64, 100, 100, p, p, p, *([p] * 16), p, ctypes.byref(hp), p, flags,
                                       ctypes.byref(lz), p, 1 << 30, None)
        assert rc == _lib.E_UNSUPPORTED, flags
        assert b"deterministic" in L.macr_last_error()


def test_unknown_flag_bits_are_invalid(L):
    from macr_amd import _lib
    for flags in (32, 32 | _lib.STEP_DETERMINISTIC, _lib.STEP_LOSS_ONLY, _lib.STEP_DENSE_LAYERS | _lib.STEP_DETERMINISTIC):
        assert _step(L, _lib.LOSS_RUBIBCEBOTH, flags) == _lib.E_INVALID, flags
        assert ("flags=%d" % flags).encode() in L.macr_last_error()


def test_per_pair_kinds_refuse_the_deferred_bits_as_before(L):
    from macr_amd import _lib
    for kind in (_lib.LOSS_NORMALBCE, _lib.LOSS_BPR):
        for seq in (_lib.STEP_DEFER, _lib.STEP_PENDING, _lib.STEP_DEFER | _lib.STEP_PENDING):
            today = _step(L, kind, seq)
            assert today == _lib.E_INVALID
            assert _step(L, kind, _lib.STEP_DETERMINISTIC | seq) == today, (kind, seq)


def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=256, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


def test_row_sharded_model_refuses_the_variable(monkeypatch):
    from macr_amd import mf
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")
    assert mf.deterministic_from_env()
    with pytest.raises(NotImplementedError, match="MACR_DETERMINISTIC"):
        mf.ShardedBPRMF(_mf_args(), dict(n_users=90, n_items=30))
    monkeypatch.setenv("MACR_DETERMINISTIC", "0")
    assert not mf.deterministic_from_env()
    monkeypatch.delenv("MACR_DETERMINISTIC")
    assert not mf.deterministic_from_env()


def test_mf_parser_gains_no_flag():
    spec = importlib.util.spec_from_file_location("mf_parse_det", os.path.join(REPO, "macr_mf", "parse.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ours = vars(mod.parse_args([]))
    assert set(ours) - set(golden("mf", "tiny")["G9"]) == {"seed", "sampler", "resume", "row_shard"}
