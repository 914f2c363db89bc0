"""Restatement of LightGCN's two item-branch losses in numpy float64: the multi-step reference of
tests/test_gpu_lgcn_branch.py (pinned to the reference's own graph code through G12 by tests/test_lgcn_branch_cpu.py).

    bce1  macr_lightgcn/LightGCN.py:432-461  si = e_i.w, sj = e_j.w on the PROPAGATED rows
    bce2  macr_lightgcn/LightGCN.py:463-493  si = e0_i.w, sj = e0_j.w on the EGO rows
    both: X[r,c] = p[c] sig(si[r]), Y[r,c] = n[c] sig(sj[r]) (the (B,) * (B,1) broadcast)
          mf  = mean(-log(sig(X)+1e-10) - log(1-sig(Y)+1e-10)) + alpha mean(-log(sig(si)+1e-10) - log(1-sig(sj)+1e-10))
          emb = decay (l2 of the ego rows) / batch_size; w moves, w_user does not
    rubi1 / rubi2 (:442 / :473): (y_ui - c) sig(e_i.w) with e_i propagated / ego
"""
import numpy as np

from bpr_ref import _sig, propagate


def lgcn_item_branch(A, T, w, n_users, n_layers, u, i, j, alpha, decay, batch_size, ego, At=None):
    """-> (loss, mf_loss, emb_loss, dT, dw) of one batch; T = [P ; Q] ego rows, ego: bce2 (else bce1)"""
    T, w = np.asarray(T, np.float64), np.asarray(w, np.float64).reshape(-1)
    At = A.T.tocsr() if At is None else At
    E = propagate(A, T, n_layers)
    iu, ii, ij = np.asarray(u), n_users + np.asarray(i), n_users + np.asarray(j)
    eu, ei, ej = E[iu], E[ii], E[ij]
    bi, bj = (T[ii], T[ij]) if ego else (ei, ej)
    B = len(u)
    p, n = (eu * ei).sum(1), (eu * ej).sum(1)
    ssi, ssj = _sig(bi @ w), _sig(bj @ w)
    sX, sY = _sig(ssi[:, None] * p[None, :]), _sig(ssj[:, None] * n[None, :])
    lo = np.mean(-np.log(sX + 1e-10) - np.log(1.0 - sY + 1e-10))
    li = np.mean(-np.log(ssi + 1e-10) - np.log(1.0 - ssj + 1e-10))
    mf = lo + alpha * li
    gu, gi, gj = T[iu], T[ii], T[ij]
    emb = decay * 0.5 * ((gu * gu).sum() + (gi * gi).sum() + (gj * gj).sum()) / batch_size
    dX = -(sX * (1.0 - sX)) / (sX + 1e-10) / (B * B)
    dY = (sY * (1.0 - sY)) / ((1.0 - sY) + 1e-10) / (B * B)
    dp, dn = (dX * ssi[:, None]).sum(0), (dY * ssj[:, None]).sum(0)
    da, db = (dX * p[None, :]).sum(1), (dY * n[None, :]).sum(1)
    dsi = (da - alpha / B / (ssi + 1e-10)) * ssi * (1.0 - ssi)
    dsj = (db + alpha / B / (1.0 - ssj + 1e-10)) * ssj * (1.0 - ssj)
    dE = np.zeros_like(T)
    np.add.at(dE, iu, dp[:, None] * ei + dn[:, None] * ej)
    np.add.at(dE, ii, dp[:, None] * eu)
    np.add.at(dE, ij, dn[:, None] * eu)
    if not ego:
        np.add.at(dE, ii, dsi[:, None] * w)
        np.add.at(dE, ij, dsj[:, None] * w)
    dT = propagate(At, dE, n_layers)                  # the gradient of mean(A^k E0) is mean((A^T)^k dE)
    if ego:                                           # the branch's rows are the ego rows themselves
        np.add.at(dT, ii, dsi[:, None] * w)
        np.add.at(dT, ij, dsj[:, None] * w)
    c = decay / batch_size
    np.add.at(dT, iu, c * gu)
    np.add.at(dT, ii, c * gi)
    np.add.at(dT, ij, c * gj)
    dw = dsi @ bi + dsj @ bj
    return mf + emb, mf, emb, dT, dw


def rubi_sig(A, T, w, n_users, n_layers, ego):
    """sig(e_i . w) of every item: the branch factor of rubi_ratings1 (propagated rows) / rubi_ratings2 (ego rows)"""
    T = np.asarray(T, np.float64)
    rows = T[n_users:] if ego else propagate(A, T, n_layers)[n_users:]
    return _sig(rows @ np.asarray(w, np.float64).reshape(-1))
