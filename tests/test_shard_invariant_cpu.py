"""The rank-count-invariant row-sharded step (MACR_SHARD_INVARIANT, include/macr_hip.h: macr_shard_*_inv) without a GPU: the new
entry points across the header, the ctypes table and the library's exports; the workspace size against the documented layout;
the slice rule; what the _inv calls refuse, next to their counterparts -- argument validation comes before any device work, so
the pointers handed in are never dereferenced (as in tests/test_shard_deterministic_cpu.py); the environment switch and its
precedence; the pinned defaults."""
import ctypes
import inspect
import os
import re
import types

import pytest

from helpers import REPO
from shard_calls import B, D, _hyper, aligned_mem, apply, backward, backward_slice, forward_slice

NEW = ("macr_shard_workspace_bytes_inv", "macr_shard_slice_inv", "macr_shard_backward_inv", "macr_shard_forward_slice_inv",
       "macr_shard_backward_slice_inv", "macr_shard_branch_fold_inv", "macr_shard_apply_inv")
ALIGN = 32


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
    assert sig["macr_shard_workspace_bytes_inv"] == sig["macr_shard_workspace_bytes"]
    assert sig["macr_shard_slice_inv"] == sig["macr_shard_slice"]
    assert sig["macr_shard_backward_inv"] == sig["macr_shard_backward"]
    assert sig["macr_shard_forward_slice_inv"] == sig["macr_shard_forward_slice"]
    assert sig["macr_shard_backward_slice_inv"] == sig["macr_shard_backward_slice"]
    assert sig["macr_shard_apply_inv"] == sig["macr_shard_apply_lazy"] == sig["macr_shard_apply_det"]
    assert len(sig["macr_shard_branch_fold_inv"][1]) == 5
    # additive: the version the existing tests pin, no new flag bit
    assert L.macr_abi_version() == 16 == lib.ABI_VERSION and re.search(r"#define MACR_ABI_VERSION\s+16\b", src)
    assert re.findall(r"#define MACR_STEP_[A-Z_]+\s+(\d+)", src) == ["1", "2", "4", "8", "16"]


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_workspace_size_is_the_documented_layout(lib, d):
    L = lib.lib()
    for b in (1, 96, 257, 300, 4096, 8448, 140000):
        plain, inv = L.macr_shard_workspace_bytes(b, d), L.macr_shard_workspace_bytes_inv(b, d)
        # the plain layout is a prefix; behind it the chunk sums (2 ceil(3B / CH) rows of d floats) and one 2 d row per backward
        # block (ceil(B / (1024 / d)) of them, 4096 at the most), each region rounded up to 256 bytes
        ch = min(d // 4, 16)
        up = lambda x: (x + 255) // 256 * 256
        assert inv == plain + up(2 * -(-3 * b // ch) * d * 4) + up(min(-(-b // (1024 // d)), 4096) * 2 * d * 4), (b, d)
        assert inv == L.macr_shard_workspace_bytes_det(b, d) and inv % 256 == 0 and plain > 0
    assert L.macr_shard_workspace_bytes_inv(0, d) == 0 and L.macr_shard_workspace_bytes_inv(-5, d) == 0
    assert L.macr_shard_workspace_bytes_inv(4096, 48) == 0


# ----------------------------------------------------------------------------- the slice rule
def slices(L, b, d, w):
    out = []
    for r in range(w):
        t0, t1 = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.macr_shard_slice_inv(b, d, r, w, ctypes.byref(t0), ctypes.byref(t1)) == 0, (b, d, w, r)
        out.append((t0.value, t1.value))
    return out


def test_slices_partition_the_batch_at_aligned_cuts_whatever_d(lib):
    L = lib.lib()
    some_empty = False
    for b in (1, 2, 5, 31, 32, 33, 64, 100, 257, 300, 777, 4096, 8192, 16384):
        for w in (1, 2, 3, 5, 8, 16):
            per_d = [slices(L, b, d, w) for d in (32, 64, 128, 256)]
            assert all(s == per_d[0] for s in per_d), (b, w)             # the rule agrees across d
            s = per_d[0]
            assert s[0][0] == 0 and s[-1][1] == b, (b, w, s)
            for (a0, a1), (b0, b1) in zip(s, s[1:]):
                assert a1 == b0 and a0 <= a1, (b, w, s)                  # consecutive, possibly empty
            for t0, t1 in s:
                assert 0 <= t0 <= t1 <= b
                assert t0 % ALIGN == 0 and (t1 % ALIGN == 0 or t1 == b), (b, w, s)
                some_empty |= t0 == t1
            # as even as the alignment allows: no slice more than one aligned block above the share
            assert max(t1 - t0 for t0, t1 in s) <= -(-(-(-b // ALIGN)) // w) * ALIGN, (b, w, s)
    assert some_empty                                                    # B < W and B = 1 are in the grid


def test_slice_inv_refuses_bad_arguments_and_too_many_blocks(lib):
    L = lib.lib()
    t0, t1 = ctypes.c_int(), ctypes.c_int()
    r0, r1 = ctypes.byref(t0), ctypes.byref(t1)
    for args in ((0, 64, 0, 2), (300, 48, 0, 2), (300, 64, 2, 2), (300, 64, -1, 2), (300, 64, 0, 0)):
        assert L.macr_shard_slice_inv(*(args + (r0, r1))) == lib.E_INVALID, args
    assert L.macr_shard_slice_inv(300, 64, 0, 2, None, r1) == lib.E_INVALID
    # the documented limit of the split form: B <= 4096 * 1024 / d
    for d in (32, 64, 128, 256):
        limit = 4096 * 1024 // d
        assert L.macr_shard_slice_inv(limit, d, 0, 2, r0, r1) == lib.OK
        assert L.macr_shard_slice_inv(limit + 1, d, 0, 2, r0, r1) == lib.E_UNSUPPORTED
        assert b"4096 blocks" in L.macr_last_error()


# ----------------------------------------------------------------------------- refusals: the codes of the counterparts
def test_backward_inv_refuses_what_backward_refuses(lib, mem):
    for over in (dict(kind=lib.LOSS_RUBIBPR), dict(kind=lib.LOSS_RUBIBCE_EGO), dict(kind=77), dict(rows3=None),
                 dict(hp=_hyper(lib, batch_size_cfg=0)), dict(hp=_hyper(lib, beta1=1.5))):
        plain = backward(lib, mem, "plain", **over)
        assert plain == lib.E_INVALID, over
        assert backward(lib, mem, "inv", **over) == plain, over
    assert backward(lib, mem, "plain", ws_bytes=16) == lib.E_WORKSPACE == backward(lib, mem, "inv", ws_bytes=16)
    assert b"workspace" in lib.lib().macr_last_error()


@pytest.mark.parametrize("call", [forward_slice, backward_slice], ids=["forward_slice", "backward_slice"])
def test_slice_calls_refuse_what_their_counterparts_refuse(lib, mem, call):
    for over, code in ((dict(kind=lib.LOSS_NORMALBCE), lib.E_UNSUPPORTED), (dict(kind=lib.LOSS_BPR), lib.E_UNSUPPORTED),
                       (dict(kind=lib.LOSS_RUBIBPR), lib.E_UNSUPPORTED), (dict(w=None), lib.E_INVALID),
                       (dict(t0=288, n=50), lib.E_INVALID), (dict(t0=-32), lib.E_INVALID), (dict(ws_bytes=16), lib.E_WORKSPACE)):
        plain = call(lib, mem, "plain", **over)
        assert plain == code, over
        assert call(lib, mem, "inv", **over) == plain, over
    # of their own: a slice not cut at multiples of 32 (the end of the batch is a cut)
    for t0, n in ((10, 54), (32, 50), (0, 299)):
        assert call(lib, mem, "plain", t0=t0, n=n, ws_bytes=16) == lib.E_WORKSPACE       # (the plain call has no such rule)
        assert call(lib, mem, "inv", t0=t0, n=n) == lib.E_INVALID, (t0, n)
    for t0, n in ((0, 0), (288, 12), (0, 300), (64, 0), (96, 204)):
        assert call(lib, mem, "inv", t0=t0, n=n, ws_bytes=16) == lib.E_WORKSPACE, (t0, n)   # accepted as a slice
    # too many blocks: refused before the workspace is looked at, nothing is launched
    for d in (32, 256):
        b = 4096 * 1024 // d + 1
        assert call(lib, mem, "inv", b=b, d=d, t0=0, n=64, ws_bytes=16) == lib.E_UNSUPPORTED
        assert b"4096 blocks" in lib.lib().macr_last_error()
        assert call(lib, mem, "inv", b=b - 1, d=d, t0=0, n=64, ws_bytes=16) == lib.E_WORKSPACE


def test_branch_fold_inv_validates_before_any_launch(lib, mem):
    L, p = lib.lib(), mem[1]
    assert L.macr_shard_branch_fold_inv(0, D, p, 1 << 30, None) == lib.E_INVALID
    assert L.macr_shard_branch_fold_inv(B, 48, p, 1 << 30, None) == lib.E_UNSUPPORTED
    assert L.macr_shard_branch_fold_inv(B, D, None, 1 << 30, None) == lib.E_INVALID
    assert L.macr_shard_branch_fold_inv(B, D, p, 16, None) == lib.E_WORKSPACE
    assert L.macr_shard_branch_fold_inv(4096 * 16 + 1, D, p, 16, None) == lib.E_UNSUPPORTED


def test_apply_inv_refuses_what_apply_refuses(lib, mem):
    for over, code in ((dict(u=None), lib.E_INVALID), (dict(n_users_loc=-1), lib.E_INVALID), (dict(ws_bytes=16), lib.E_WORKSPACE)):
        assert apply(lib, mem, "plain", **over) == code == apply(lib, mem, "inv", **over), over
        assert apply(lib, mem, "lazy", **over) == code == apply(lib, mem, "inv_lazy", **over), over
    for period in (0, 65):                                  # the lazy form's own checks, when lazy is given
        assert apply(lib, mem, "lazy", lazy_period=period) == lib.E_INVALID == apply(lib, mem, "inv_lazy", lazy_period=period)
        assert apply(lib, mem, "inv", lazy_period=period, ws_bytes=16) == lib.E_WORKSPACE     # lazy = NULL: nothing to check there


def test_inv_calls_refuse_a_workspace_of_the_plain_size(lib, mem):
    L = lib.lib()
    plain, inv = L.macr_shard_workspace_bytes(B, D), L.macr_shard_workspace_bytes_inv(B, D)
    assert inv > plain
    for rc in (backward(lib, mem, "inv", ws_bytes=plain), backward(lib, mem, "inv", kind=lib.LOSS_NORMALBCE, ws_bytes=plain),
               forward_slice(lib, mem, "inv", ws_bytes=plain), backward_slice(lib, mem, "inv", ws_bytes=plain),
               apply(lib, mem, "inv", ws_bytes=plain), apply(lib, mem, "inv_lazy", ws_bytes=plain),
               L.macr_shard_branch_fold_inv(B, D, mem[1], plain, None), backward(lib, mem, "inv", ws_bytes=inv - 1)):
        assert rc == lib.E_WORKSPACE
        assert b"workspace" in L.macr_last_error()


# ----------------------------------------------------------------------------- the switch
def _mf_args():
    return types.SimpleNamespace(regs=1e-5, embed_size=64, lr=1e-3, batch_size=256, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)


def test_switch_reads_the_environment(monkeypatch):
    from macr_amd import sharded_train
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC", raising=False)
    monkeypatch.setenv("MACR_SHARD_INVARIANT", "1")
    assert sharded_train.shard_invariant_from_env()
    assert not sharded_train.shard_deterministic_from_env()           # a switch of its own
    monkeypatch.setenv("MACR_SHARD_INVARIANT", "0")
    assert not sharded_train.shard_invariant_from_env()
    monkeypatch.delenv("MACR_SHARD_INVARIANT")
    assert not sharded_train.shard_invariant_from_env()
    for other in ("MACR_SHARD_DETERMINISTIC", "MACR_DETERMINISTIC"):   # the other switches are not this one
        monkeypatch.setenv(other, "1")
        assert not sharded_train.shard_invariant_from_env()


def test_backend_keyword_and_precedence():
    """the invariant mode wins over the deterministic one in the backend (no device is touched: nothing is reserved before the
    first step)"""
    from macr_amd import _lib, sharded_train
    params = inspect.signature(sharded_train.HipBackend.__init__).parameters
    assert params["deterministic"].default is False and params["invariant"].default is False
    assert list(params)[:7] == ["self", "kind", "d", "hyper", "device", "deterministic", "invariant"]
    hp = _hyper(_lib)
    hp.beta1, hp.beta2 = 0.9, 0.999
    for det, inv, want in ((False, False, (False, False)), (True, False, (True, False)), (False, True, (False, True)),
                           (True, True, (False, True))):
        be = sharded_train.HipBackend(_lib.LOSS_RUBIBCEBOTH, 64, hp, "cpu", deterministic=det, invariant=inv)
        assert (be.deterministic, be.invariant) == want


def test_model_takes_the_mode_from_its_backend():
    import torch

    from macr_amd import sharded_train
    P, Q, w = torch.zeros(6, 4), torch.zeros(5, 4), torch.zeros(4)
    for mode in (True, False):
        m = sharded_train.RowShardedMF(P, Q, w, w, types.SimpleNamespace(invariant=mode), rank=0, world=1)
        assert m.invariant is mode and m.deterministic is False
    assert sharded_train.RowShardedMF(P, Q, w, w, types.SimpleNamespace(), rank=0, world=1).invariant is False


def test_sharded_model_defaults_and_environment(monkeypatch):
    import torch

    from macr_amd import mf
    params = inspect.signature(mf.ShardedBPRMF.__init__).parameters
    assert params["deterministic"].default is None and params["invariant"].default is None
    cfg, cpu = dict(n_users=90, n_items=30), torch.device("cpu")
    for name in ("MACR_SHARD_INVARIANT", "MACR_SHARD_DETERMINISTIC", "MACR_DETERMINISTIC", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(name, raising=False)
    m = mf.ShardedBPRMF(_mf_args(), cfg, device=cpu)
    assert not m.invariant and not m.deterministic
    monkeypatch.setenv("MACR_SHARD_INVARIANT", "1")
    m = mf.ShardedBPRMF(_mf_args(), cfg, device=cpu)
    assert m.invariant and not m.deterministic
    assert not mf.ShardedBPRMF(_mf_args(), cfg, device=cpu, invariant=False).invariant       # the keyword decides over the variable
    monkeypatch.setenv("MACR_SHARD_DETERMINISTIC", "1")                                      # both: the invariant mode wins
    m = mf.ShardedBPRMF(_mf_args(), cfg, device=cpu)
    assert m.invariant
    assert m._model(m.kind_of("rubibceboth")).invariant and not m._model(m.kind_of("rubibceboth")).deterministic
    monkeypatch.delenv("MACR_SHARD_DETERMINISTIC")
    monkeypatch.setenv("MACR_DETERMINISTIC", "1")                  # implies the deterministic promises: the unsharded switch is served
    assert mf.ShardedBPRMF(_mf_args(), cfg, device=cpu).invariant
    monkeypatch.delenv("MACR_SHARD_INVARIANT")
    with pytest.raises(NotImplementedError, match="MACR_SHARD_DETERMINISTIC"):
        mf.ShardedBPRMF(_mf_args(), cfg, device=cpu)


def test_cli_names_the_switch_in_its_refusal():
    src = open(os.path.join(REPO, "macr_mf", "train.py")).read()
    assert 'os.environ.get("MACR_SHARD_INVARIANT", "") == "1"' in src and "add --row_shard 1" in src
