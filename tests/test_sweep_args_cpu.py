"""macr_score_topk_sweep's refusals and its workspace size, without a GPU: argument validation comes before any device work
(the pointers below are never dereferenced; tests/test_rubi_bpr_cpu.py relies on the same order for the training entry
points), so every documented error code can be asserted on any machine."""
import ctypes

import pytest

U, N, D, K = 300, 2500, 64, 20


@pytest.fixture(scope="module")
def lib():
    from macr_amd import _lib
    from macr_amd.build import build
    build()
    return _lib


@pytest.fixture(scope="module")
def mem():
    """a 256-byte aligned host address standing in for every buffer"""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, base


def call(lib, mem, **over):
    """the sweep with valid arguments but for `over` -> return code"""
    p = ctypes.c_void_p(mem[1])
    L = lib.lib()
    a = dict(kind=lib.SCORE_RUBI_BOTH, filter=1, U=U, N=N, d=D, users=p, user_ids=p, items=p, sig_u=p, sig_i=p, n_c=3, c_dev=p,
             mask_ptr=p, mask_idx=p, mask_bits=p, off=0, K=K, out_val=p, out_idx=p, ws=p, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.macr_score_topk_sweep_workspace_bytes(a["U"], a["N"], a["d"] if a["d"] in (32, 64, 128, 256) else 64,
                                                                min(max(a["n_c"], 1), lib.MAX_SWEEP))
    return L.macr_score_topk_sweep(a["kind"], a["filter"], a["U"], a["N"], a["d"], a["users"], a["user_ids"], a["items"], a["sig_u"],
                                   a["sig_i"], a["n_c"], a["c_dev"], a["mask_ptr"], a["mask_idx"], a["mask_bits"], a["off"], a["K"],
                                   a["out_val"], a["out_idx"], a["ws"], a["ws_bytes"], None)


def test_sweep_refuses_with_its_documented_codes(lib, mem):
    L = lib.lib()
    refused = [
        ("a kind that does not read c", dict(kind=lib.SCORE_NORMAL), lib.E_INVALID, b"does not depend on c"),
        ("no kind at all", dict(kind=5), lib.E_INVALID, b"score_kind=5"),
        ("n_c = 0", dict(n_c=0), lib.E_UNSUPPORTED, b"n_c=0"),
        ("n_c = 5", dict(n_c=lib.MAX_SWEEP + 1), lib.E_UNSUPPORTED, b"n_c=5"),
        ("K = 0", dict(K=0), lib.E_UNSUPPORTED, b"K=0"),
        ("K = 33", dict(K=lib.MAX_TOPK_FUSED + 1), lib.E_UNSUPPORTED, b"K=33"),
        ("d = 48", dict(d=48), lib.E_UNSUPPORTED, b"d=48"),
        ("a mask without its bitmap", dict(mask_bits=None), lib.E_INVALID, b"mask bitmap"),
        ("an unaligned workspace", dict(ws=ctypes.c_void_p(mem[1] + 64)), lib.E_INVALID, b"workspace"),
        ("no workspace", dict(ws=None), lib.E_INVALID, b"workspace"),
        ("a workspace one byte short", dict(ws_bytes=L.macr_score_topk_sweep_workspace_bytes(U, N, D, 3) - 1), lib.E_WORKSPACE,
         b"workspace"),
        ("the workspace of two values for three", dict(ws_bytes=L.macr_score_topk_sweep_workspace_bytes(U, N, D, 2)),
         lib.E_WORKSPACE, b"workspace"),
        ("RUBI_BOTH without sig_u", dict(sig_u=None), lib.E_INVALID, b"null pointer"),
        ("DIRECT_MINUS_BOTH without sig_u", dict(kind=lib.SCORE_DIRECT_MINUS_BOTH, sig_u=None), lib.E_INVALID, b"null pointer"),
        ("no sig_i", dict(kind=lib.SCORE_RUBI, sig_i=None), lib.E_INVALID, b"null pointer"),
        ("no values of c", dict(c_dev=None), lib.E_INVALID, b"null pointer"),
    ]
    for name, over, code, text in refused:
        rc = call(lib, mem, **over)
        assert rc == code, (name, rc, L.macr_last_error())
        msg = L.macr_last_error()
        assert b"score_topk_sweep" in msg and text in msg, (name, msg)


def test_one_branch_kinds_need_no_sig_u(lib, mem):
    """RUBI and DIRECT_MINUS without sig_u pass the pointer check: the call gets as far as the workspace check"""
    for kind in (lib.SCORE_RUBI, lib.SCORE_DIRECT_MINUS):
        assert call(lib, mem, kind=kind, sig_u=None, ws_bytes=256) == lib.E_WORKSPACE, lib.lib().macr_last_error()
    # ... and so does a call without mask and without query ids
    assert call(lib, mem, mask_ptr=None, mask_idx=None, mask_bits=None, user_ids=None, ws_bytes=256) == lib.E_WORKSPACE


def test_sweep_workspace_is_one_ranking_workspace_per_value(lib):
    L = lib.lib()
    ws = L.macr_score_topk_sweep_workspace_bytes
    for u, n, d in [(U, N, D), (1, 5, 32), (257, 1024, 128), (700, 8993, 256), (33, 1025, 256)]:
        one = ws(u, n, d, 1)
        assert one > 0 and one % 256 == 0
        assert one >= L.macr_score_topk_workspace_bytes(u, n, d)             # a value's slice holds a whole ranking workspace
        for n_c in range(1, lib.MAX_SWEEP + 1):
            assert ws(u, n, d, n_c) == n_c * one, (u, n, d, n_c)
    for bad in [(0, N, D, 2), (U, 0, D, 2), (-1, N, D, 2), (U, N, 48, 2), (U, N, D, 0), (U, N, D, lib.MAX_SWEEP + 1), (U, N, D, -1)]:
        assert ws(*bad) == 0, bad
