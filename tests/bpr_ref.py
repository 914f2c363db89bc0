"""Restatement of the two BPR losses and of tf.train.AdamOptimizer's dense rule, in numpy float64: the multi-step reference
of tests/test_gpu_bpr.py (pinned to the reference's own graph code through G11 by tests/test_bpr_cpu.py).

    mf_bpr    macr_mf/model.py:264-275      mf = -mean(log(sig(p - n))), reg = decay * (l2(e_u) + l2(e_i) + l2(e_j)) / batch_size
    lgcn_bpr  macr_lightgcn/LightGCN.py:398-413 on the propagated rows (:288-309), regulariser on the ego rows:
              mf = -mean(log(1e-9 + sig(sig(p) - sig(n)))), emb = decay * (l2 of the ego rows) / batch_size
    adam      the rule orc_adam_dense (oracle/macr_oracle.c) states: m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2,
              theta -= lr_t m / (sqrt(v) + eps), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); every row moves every step
"""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def mf_bpr(P, Q, u, i, j, decay, batch_size):
    """-> (loss, mf_loss, reg_loss, dP, dQ) of one batch"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    eu, ei, ej = P[u], Q[i], Q[j]
    B = len(u)
    p, n = (eu * ei).sum(1), (eu * ej).sum(1)
    s = _sig(p - n)
    mf = -np.mean(np.log(s))
    reg = decay * 0.5 * ((eu * eu).sum() + (ei * ei).sum() + (ej * ej).sum()) / batch_size
    g = (-(1.0 - s) / B)[:, None]                    # d mf / d (p - n)
    c = decay / batch_size
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(dP, u, g * (ei - ej) + c * eu)
    np.add.at(dQ, i, g * eu + c * ei)
    np.add.at(dQ, j, -g * eu + c * ej)
    return mf + reg, mf, reg, dP, dQ


def propagate(A, E0, n_layers):
    """mean(E0, A E0, ..., A^L E0) (LightGCN.py:288-309); A: scipy sparse"""
    E, acc = E0, E0.copy()
    for _ in range(n_layers):
        E = A @ E
        acc = acc + E
    return acc / (n_layers + 1)


def lgcn_bpr(A, T, n_users, n_layers, u, i, j, decay, batch_size, At=None):
    """-> (loss, mf_loss, emb_loss, dT) of one batch; T = [P ; Q] ego rows, At: the transposed adjacency (None: A)"""
    T = np.asarray(T, np.float64)
    At = A.T.tocsr() if At is None else At
    E = propagate(A, T, n_layers)
    iu, ii, ij = np.asarray(u), n_users + np.asarray(i), n_users + np.asarray(j)
    eu, ei, ej = E[iu], E[ii], E[ij]
    B = len(u)
    sp, sn = _sig((eu * ei).sum(1)), _sig((eu * ej).sum(1))
    y = _sig(sp - sn)
    mf = -np.mean(np.log(1e-9 + y))
    gu, gi, gj = T[iu], T[ii], T[ij]
    emb = decay * 0.5 * ((gu * gu).sum() + (gi * gi).sum() + (gj * gj).sum()) / batch_size
    g = -(y * (1.0 - y)) / (y + 1e-9) / B
    dp, dn = (g * sp * (1.0 - sp))[:, None], (-g * sn * (1.0 - sn))[:, None]
    dE = np.zeros_like(T)
    np.add.at(dE, iu, dp * ei + dn * ej)
    np.add.at(dE, ii, dp * eu)
    np.add.at(dE, ij, dn * eu)
    dT = propagate(At, dE, n_layers)                  # the gradient of mean(A^k E0) is mean((A^T)^k dE)
    c = decay / batch_size
    np.add.at(dT, iu, c * gu)
    np.add.at(dT, ii, c * gi)
    np.add.at(dT, ij, c * gj)
    return mf + emb, mf, emb, dT


class Adam(object):
    """dense tf.train.AdamOptimizer over a list of float64 arrays"""

    def __init__(self, params, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.params = [np.array(p, np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.params]
        self.v = [np.zeros_like(p) for p in self.params]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, b1, b2, eps, 0

    def step(self, grads):
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for p, m, v, g in zip(self.params, self.m, self.v, grads):
            m *= self.b1
            m += (1.0 - self.b1) * g
            v *= self.b2
            v += (1.0 - self.b2) * g * g
            p -= lr_t * m / (np.sqrt(v) + self.eps)
