"""The bit-reproducible row-sharded step (MACR_SHARD_DETERMINISTIC, include/macr_hip.h: macr_shard_*_det) without a GPU: the new
entry points across the header, the ctypes table and the library's exports; the workspace size function; what the _det calls
refuse, next to their plain counterparts; the environment switch.  Argument validation comes before any device work, so the
pointers handed in are never dereferenced (as in tests/test_deterministic_cpu.py)."""
import functools
import os
import re
import types

import pytest

import shard_calls
from helpers import REPO
from shard_calls import B, D, _hyper, aligned_mem, apply, backward

backward_slice = functools.partial(shard_calls.backward_slice, t0=10, n=50)      # (a slice that begins at no block boundary)

NEW = ("macr_shard_workspace_bytes_det", "macr_shard_backward_det", "macr_shard_backward_slice_det", "macr_shard_apply_det",
       "macr_shard_fold_ranks")


@pytest.fixture(scope="module")
def lib():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    return aligned_mem()


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported(lib):
    L = lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "macr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(macr_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared and name in lib.SIGNATURES and hasattr(L, name), name
    assert sorted(lib.SIGNATURES) == sorted(declared)
    sig = lib.SIGNATURES
    # arguments as the plain counterparts; apply_det = apply_lazy (lazy nullable)
    assert sig["macr_shard_backward_det"] == sig["macr_shard_backward"]
    assert sig["macr_shard_backward_slice_det"] == sig["macr_shard_backward_slice"]
    assert sig["macr_shard_apply_det"] == sig["macr_shard_apply_lazy"]
    assert sig["macr_shard_workspace_bytes_det"] == sig["macr_shard_workspace_bytes"]
    assert len(sig["macr_shard_fold_ranks"][1]) == 5
    # additive: the version the existing tests pin, no new flag bit
    assert L.macr_abi_version() == 16 == lib.ABI_VERSION and re.search(r"#define MACR_ABI_VERSION\s+16\b", src)
    assert re.findall(r"#define MACR_STEP_[A-Z_]+\s+(\d+)", src) == ["1", "2", "4", "8", "16"]


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_workspace_size_function(lib, d):
    L = lib.lib()
    for b in (1, 96, 257, 300, 4096, 8448):
        plain, det = L.macr_shard_workspace_bytes(b, d), L.macr_shard_workspace_bytes_det(b, d)
        assert det >= plain > 0, (b, d)
        # the plain layout is a prefix; behind it the chunk sums (2 ceil(3B / CH) rows of d floats) and one 2 d row per backward
        # block (ceil(B / (1024 / d)) of them below 4096), each region rounded up to 256 bytes
        ch = min(d // 4, 16)
        up = lambda x: (x + 255) // 256 * 256
        assert det == plain + up(2 * -(-3 * b // ch) * d * 4) + up(min(-(-b // (1024 // d)), 4096) * 2 * d * 4), (b, d)
        assert det % 256 == 0
    assert L.macr_shard_workspace_bytes_det(0, d) == 0 and L.macr_shard_workspace_bytes_det(-5, d) == 0


def test_workspace_size_is_zero_for_an_unsupported_width(lib):
    L = lib.lib()
    assert L.macr_shard_workspace_bytes_det(4096, 48) == 0 == L.macr_shard_workspace_bytes(4096, 48)


# ----------------------------------------------------------------------------- refusals: the codes of the plain calls
def test_backward_det_refuses_what_backward_refuses(lib, mem):
    for over in (dict(kind=lib.LOSS_RUBIBPR), dict(kind=lib.LOSS_RUBIBCE_EGO), dict(kind=77), dict(rows3=None),
                 dict(hp=_hyper(lib, batch_size_cfg=0)), dict(hp=_hyper(lib, beta1=1.5))):
        plain = backward(lib, mem, "plain", **over)
        assert plain == lib.E_INVALID, over
        assert backward(lib, mem, "det", **over) == plain, over
    assert backward(lib, mem, "plain", ws_bytes=16) == lib.E_WORKSPACE == backward(lib, mem, "det", ws_bytes=16)
    assert b"workspace" in lib.lib().macr_last_error()


def test_backward_slice_det_refuses_what_backward_slice_refuses(lib, mem):
    for over, code in ((dict(kind=lib.LOSS_NORMALBCE), lib.E_UNSUPPORTED), (dict(kind=lib.LOSS_BPR), lib.E_UNSUPPORTED),
                       (dict(kind=lib.LOSS_RUBIBPR), lib.E_UNSUPPORTED), (dict(w=None), lib.E_INVALID),
                       (dict(t0=280, n=50), lib.E_INVALID), (dict(t0=-1), lib.E_INVALID), (dict(ws_bytes=16), lib.E_WORKSPACE)):
        plain = backward_slice(lib, mem, "plain", **over)
        assert plain == code, over
        assert backward_slice(lib, mem, "det", **over) == plain, over


def test_apply_det_refuses_what_apply_refuses(lib, mem):
    for over, code in ((dict(u=None), lib.E_INVALID), (dict(n_users_loc=-1), lib.E_INVALID), (dict(ws_bytes=16), lib.E_WORKSPACE)):
        assert apply(lib, mem, "plain", **over) == code == apply(lib, mem, "det", **over), over
        assert apply(lib, mem, "lazy", **over) == code == apply(lib, mem, "det_lazy", **over), over
    for period in (0, 65):                                  # the lazy form's own checks, when lazy is given
        assert apply(lib, mem, "lazy", lazy_period=period) == lib.E_INVALID == apply(lib, mem, "det_lazy", lazy_period=period)
        assert apply(lib, mem, "det", lazy_period=period, ws_bytes=16) == lib.E_WORKSPACE     # lazy = NULL: nothing to check there


def test_det_calls_refuse_a_workspace_of_the_plain_size(lib, mem):
    L = lib.lib()
    plain, det = L.macr_shard_workspace_bytes(B, D), L.macr_shard_workspace_bytes_det(B, D)
    assert det > plain
    # (the plain calls reach their launches with this size: not called here, there is no device)
    for rc in (backward(lib, mem, "det", ws_bytes=plain), backward(lib, mem, "det", kind=lib.LOSS_NORMALBCE, ws_bytes=plain),
               backward_slice(lib, mem, "det", ws_bytes=plain), apply(lib, mem, "det", ws_bytes=plain),
               apply(lib, mem, "det_lazy", ws_bytes=plain), backward(lib, mem, "det", ws_bytes=det - 1)):
        assert rc == lib.E_WORKSPACE
        assert b"workspace" in L.macr_last_error()


def test_fold_ranks_validates_before_any_launch(lib, mem):
    L, p = lib.lib(), mem[1]
    assert L.macr_shard_fold_ranks(0, 16, p, p, None) == lib.E_INVALID
    assert L.macr_shard_fold_ranks(3, -1, p, p, None) == lib.E_INVALID
    assert L.macr_shard_fold_ranks(3, 16, None, p, None) == lib.E_INVALID
    assert L.macr_shard_fold_ranks(3, 16, p, None, None) == lib.E_INVALID
    assert L.macr_shard_fold_ranks(3, 0, None, None, None) == lib.OK          # nothing to fold: no launch


# ----------------------------------------------------------------------------- the switch
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=256, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


def test_switch_reads_the_environment(monkeypatch):
    from macr_amd import sharded_train
    monkeypatch.setenv("MACR_SHARD_DETERMINISTIC", "1")
    assert sharded_train.shard_deterministic_from_env()
    monkeypatch.setenv("MACR_SHARD_DETERMINISTIC", "0")
    assert not sharded_train.shard_deterministic_from_env()
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC")
    assert not sharded_train.shard_deterministic_from_env()
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")           # the other switch is not this one
    assert not sharded_train.shard_deterministic_from_env()


def test_the_unsharded_switch_alone_still_refuses_and_names_the_new_one(monkeypatch):
    from macr_amd import mf
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC", raising=False)
    with pytest.raises(NotImplementedError, match="MACR_SHARD_DETERMINISTIC"):
        mf.ShardedBPRMF(_mf_args(), dict(n_users=90, n_items=30))
    with pytest.raises(NotImplementedError, match="MACR_DETERMINISTIC=1"):
        mf.ShardedBPRMF(_mf_args(), dict(n_users=90, n_items=30))


def test_backend_and_model_carry_the_mode():
    """the keyword reaches the backend, and RowShardedMF takes the mode from its backend (no device is touched here: a CPU
    stand-in for the backend, CPU tensors)"""
    import inspect

    import torch

    from macr_amd import mf, sharded_train
    assert inspect.signature(sharded_train.HipBackend.__init__).parameters["deterministic"].default is False
    assert inspect.signature(mf.ShardedBPRMF.__init__).parameters["deterministic"].default is None
    P, Q, w = torch.zeros(6, 4), torch.zeros(5, 4), torch.zeros(4)
    for mode in (True, False):
        m = sharded_train.RowShardedMF(P, Q, w, w, types.SimpleNamespace(deterministic=mode), rank=0, world=1)
        assert m.deterministic is mode
    assert sharded_train.RowShardedMF(P, Q, w, w, types.SimpleNamespace(), rank=0, world=1).deterministic is False
