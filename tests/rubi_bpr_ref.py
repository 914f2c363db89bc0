"""Restatement of the MF two-branch BPR loss (`--train rubi`, MACR_LOSS_RUBIBPR) in numpy float64: the multi-step reference of
tests/test_gpu_rubi_bpr.py, pinned to the reference's own graph code through G13 by tests/test_rubi_bpr_cpu.py.  Adam is
bpr_ref.Adam (params P, Q, w; w_user is not trained).

    create_bpr_loss_two_brach  macr_mf/model.py:124-156, trained by opt_two (:64-66)
        p = e_u.e_i, n = e_u.e_j, s_i = e_i.w, s_j = e_j.w, a = sig(s_i), b = sig(s_j)
        Z[r,c] = a[r] p[c] - b[r] n[c]            (a (B,) score vector times a (B,1) sigmoid: a (B,B) matrix, :138-140)
        mf  = -mean_{r,c} log(sig(Z)) - alpha mean_r log(sig(s_i - s_j))          (no epsilon)
        reg = decay (l2(e_u) + l2(e_i) + l2(e_j)) / batch_size

The (B,B) matrix is walked in row slabs (B = 2^17 is 1.7e10 cells: 137 GB at once), on a few threads (numpy's loops
release the GIL).  `device` moves the slab arithmetic -- the same float64 expressions -- to torch on that device: the tests
of the largest batches pass "cuda" (minutes of host time otherwise); tests/test_rubi_bpr_cpu.py pins it to the numpy form.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_SLAB_CELLS = 1 << 22


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _neglog_sig(x):
    """-log(sig(x)) = log(1 + e^-x), stable for the x of the tests (|x| < 700)"""
    return np.logaddexp(0.0, -x)


def mf_problem(seed, n_users, n_items, d, B, scale):
    """tests/golden/make_golden_model.py::mf_problem, restated (G13's case d inputs pin it): P, Q, w, wu, u, i, j"""
    rs = np.random.RandomState(seed)
    P = (rs.standard_normal((n_users, d)) * scale).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * scale).astype(np.float32)
    w = (rs.standard_normal((d, 1)) * 0.3).astype(np.float32)
    wu = (rs.standard_normal((d, 1)) * 0.3).astype(np.float32)
    u = rs.choice(n_users, B, replace=B > n_users).astype(np.int64)
    i = rs.randint(0, n_items, B).astype(np.int64)
    j = rs.randint(0, n_items, B).astype(np.int64)
    i[: B // 3] = 0
    return P, Q, w, wu, u, i, j


def z_matrix(P, Q, w, u, i, j):
    P, Q, w = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(w, np.float64).reshape(-1)
    eu, ei, ej = P[u], Q[i], Q[j]
    a, b = _sig(ei @ w), _sig(ej @ w)
    return a[:, None] * (eu * ei).sum(1)[None, :] - b[:, None] * (eu * ej).sum(1)[None, :]


def _bxb_torch(a, b, p, n, device):
    import torch
    B = len(a)
    ta, tb, tp, tn = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (a, b, p, n))
    rows = max(1, (1 << 26) // B)
    lsum = torch.zeros((), dtype=torch.float64, device=device)
    ga, gb = torch.zeros_like(ta), torch.zeros_like(ta)
    gp, gn = torch.zeros_like(ta), torch.zeros_like(ta)
    for r0 in range(0, B, rows):
        r1 = min(B, r0 + rows)
        Z = ta[r0:r1, None] * tp[None, :] - tb[r0:r1, None] * tn[None, :]
        nl = torch.logaddexp(torch.zeros_like(Z), -Z)
        g = torch.exp(-Z - nl)
        lsum += nl.sum()
        ga += ta[r0:r1] @ g
        gb += tb[r0:r1] @ g
        gp[r0:r1], gn[r0:r1] = g @ tp, g @ tn
    return (float(lsum),) + tuple(x.cpu().numpy() for x in (ga, gb, gp, gn))


def _bxb(a, b, p, n, device=None):
    """the (B,B) term: sum of -log(sig(Z)) and the sums of g = 1 - sig(Z) against a, b (per column) and p, n (per row)"""
    if device is not None:
        return _bxb_torch(a, b, p, n, device)
    B = len(a)
    rows = max(1, _SLAB_CELLS // B)

    def slab(r0):
        r1 = min(B, r0 + rows)
        Z = a[r0:r1, None] * p[None, :] - b[r0:r1, None] * n[None, :]
        nl = _neglog_sig(Z)
        g = np.exp(-Z - nl)                            # 1 - sig(Z) = e^-Z / (1 + e^-Z)
        return r0, r1, nl.sum(), a[r0:r1] @ g, b[r0:r1] @ g, g @ p, g @ n

    starts = range(0, B, rows)
    if len(starts) > 1:
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            parts = list(pool.map(slab, starts))
    else:
        parts = [slab(r0) for r0 in starts]
    lsum, ga, gb = 0.0, np.zeros(B), np.zeros(B)
    gp, gn = np.zeros(B), np.zeros(B)
    for r0, r1, l, ca, cb_, rp, rn in parts:
        lsum += l
        ga += ca
        gb += cb_
        gp[r0:r1], gn[r0:r1] = rp, rn
    return lsum, ga, gb, gp, gn


def mf_rubi_bpr(P, Q, w, u, i, j, alpha, decay, batch_size, device=None):
    """-> (loss, mf_loss, reg_loss, dP, dQ, dw) of one batch"""
    P, Q, w = np.asarray(P, np.float64), np.asarray(Q, np.float64), np.asarray(w, np.float64).reshape(-1)
    eu, ei, ej = P[u], Q[i], Q[j]
    B = len(u)
    p, n = (eu * ei).sum(1), (eu * ej).sum(1)
    si, sj = ei @ w, ej @ w
    a, b = _sig(si), _sig(sj)
    lsum, ga, gb, gp, gn = _bxb(a, b, p, n, device)
    mf = lsum / (B * B) + alpha * _neglog_sig(si - sj).mean()
    reg = decay * 0.5 * ((eu * eu).sum() + (ei * ei).sum() + (ej * ej).sum()) / batch_size
    # G = d L_ori / d Z = -g / B^2:  dp[c] = sum_r G a[r], dn[c] = -sum_r G b[r], da[r] = sum_c G p[c], db[r] = -sum_c G n[c]
    s = 1.0 / (B * B)
    dp, dn, da, db = -ga * s, gb * s, -gp * s, gn * s
    h = (1.0 - _sig(si - sj)) / B
    dsi, dsj = da * a * (1.0 - a) - alpha * h, db * b * (1.0 - b) + alpha * h
    c = decay / batch_size
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(dP, u, dp[:, None] * ei + dn[:, None] * ej + c * eu)
    np.add.at(dQ, i, dp[:, None] * eu + dsi[:, None] * w[None, :] + c * ei)
    np.add.at(dQ, j, dn[:, None] * eu + dsj[:, None] * w[None, :] + c * ej)
    dw = dsi @ ei + dsj @ ej
    return mf + reg, mf, reg, dP, dQ, dw
