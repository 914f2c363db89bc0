"""Restatement of LightGCN's `--loss bce` and `--loss bceboth` in numpy float64: the multi-step reference of
tests/test_gpu_lgcn_trajectory.py (pinned to the reference's own graph code through G10 by tests/test_lgcn_both_cpu.py).

    bce      macr_lightgcn/LightGCN.py:415-429  mf = mean(-log(sig(p)+1e-9) - log(1-sig(n)+1e-9)), p = e_u.e_i, n = e_u.e_j
                                                on the PROPAGATED rows; w and w_user are not in the graph
    bceboth  macr_lightgcn/LightGCN.py:495-532  si = e_i.w, sj = e_j.w, su = e_u.w_user, all on the PROPAGATED rows
             X[r,c] = p[c] sig(si[r]) sig(su[r]), Y[r,c] = n[c] sig(sj[r]) sig(su[r]) (the (B,) * (B,1) * (B,1) broadcast)
             mf = mean(-log(sig(X)+1e-10) - log(1-sig(Y)+1e-10)) + alpha mean(-log(sig(si)+1e-10) - log(1-sig(sj)+1e-10))
                  + beta mean(-log(sig(su)+1e-10) - log(1-sig(su)+1e-10))
    both: emb = decay (l2 of the EGO rows) / batch_size

and the twenty-step problems both test files run (problem / reference, built once per case)."""
import functools

import numpy as np

from bpr_ref import Adam, _sig, propagate


def lgcn_both(A, T, w, wu, n_users, n_layers, u, i, j, alpha, beta, decay, batch_size, both, At=None):
    """-> (loss, mf_loss, emb_loss, dT, dw, dwu) of one batch; T = [P ; Q] ego rows, At: the transposed adjacency (None: A^T),
    both: bceboth -- else bce, whose dw and dwu are zero: neither vector is in its graph, and tf.train.AdamOptimizer leaves a
    variable without a gradient and its slots alone (the caller must not step them)"""
    T = np.asarray(T, np.float64)
    w, wu = np.asarray(w, np.float64).reshape(-1), np.asarray(wu, np.float64).reshape(-1)
    At = A.T.tocsr() if At is None else At
    E = propagate(A, T, n_layers)
    iu, ii, ij = np.asarray(u), n_users + np.asarray(i), n_users + np.asarray(j)
    eu, ei, ej = E[iu], E[ii], E[ij]
    B = len(u)
    p, n = (eu * ei).sum(1), (eu * ej).sum(1)
    dE = np.zeros_like(T)
    if both:
        ssi, ssj, ssu = _sig(ei @ w), _sig(ej @ w), _sig(eu @ wu)
        a, b = ssi * ssu, ssj * ssu                      # the row factors of X and Y
        sX, sY = _sig(a[:, None] * p[None, :]), _sig(b[:, None] * n[None, :])
        lo = np.mean(-np.log(sX + 1e-10) - np.log(1.0 - sY + 1e-10))
        li = np.mean(-np.log(ssi + 1e-10) - np.log(1.0 - ssj + 1e-10))
        lu = np.mean(-np.log(ssu + 1e-10) - np.log(1.0 - ssu + 1e-10))
        mf = lo + alpha * li + beta * lu
        dX = -(sX * (1.0 - sX)) / (sX + 1e-10) / (B * B)
        dY = (sY * (1.0 - sY)) / ((1.0 - sY) + 1e-10) / (B * B)
        dp, dn = (dX * a[:, None]).sum(0), (dY * b[:, None]).sum(0)
        da, db = (dX * p[None, :]).sum(1), (dY * n[None, :]).sum(1)
        dsi = (da * ssu - alpha / B / (ssi + 1e-10)) * ssi * (1.0 - ssi)
        dsj = (db * ssu + alpha / B / (1.0 - ssj + 1e-10)) * ssj * (1.0 - ssj)
        dsu = (da * ssi + db * ssj + beta / B * (1.0 / (1.0 - ssu + 1e-10) - 1.0 / (ssu + 1e-10))) * ssu * (1.0 - ssu)
        np.add.at(dE, iu, dsu[:, None] * wu)
        np.add.at(dE, ii, dsi[:, None] * w)
        np.add.at(dE, ij, dsj[:, None] * w)
        dw, dwu = dsi @ ei + dsj @ ej, dsu @ eu
    else:
        sp, sn = _sig(p), _sig(n)
        mf = np.mean(-np.log(sp + 1e-9) - np.log(1.0 - sn + 1e-9))
        dp = -(sp * (1.0 - sp)) / (sp + 1e-9) / B
        dn = (sn * (1.0 - sn)) / ((1.0 - sn) + 1e-9) / B
        dw, dwu = np.zeros_like(w), np.zeros_like(wu)
    gu, gi, gj = T[iu], T[ii], T[ij]
    emb = decay * 0.5 * ((gu * gu).sum() + (gi * gi).sum() + (gj * gj).sum()) / batch_size
    np.add.at(dE, iu, dp[:, None] * ei + dn[:, None] * ej)
    np.add.at(dE, ii, dp[:, None] * eu)
    np.add.at(dE, ij, dn[:, None] * eu)
    dT = propagate(At, dE, n_layers)                  # the gradient of mean(A^k E0) is mean((A^T)^k dE)
    c = decay / batch_size
    np.add.at(dT, iu, c * gu)
    np.add.at(dT, ii, c * gi)
    np.add.at(dT, ij, c * gj)
    return mf + emb, mf, emb, dT, dw, dwu


# ----------------------------------------------------------------------------- the twenty-step problems
LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 1024          # (those of tests/test_gpu_lgcn_branch.py)
STEPS = 20
N_USERS, N_ITEMS = 500, 300
SLOTS = ("mT", "vT", "mw", "vw", "mwu", "vwu")


@functools.lru_cache(maxsize=None)
def problem(asym, n_layers, d, B):
    """the graph of test_gpu_lgcn_branch.lgcn_graph (500 users x 300 items, D^-1/2 A D^-1/2, asym: D^-1 A), a table, two
    branch vectors and STEPS + 1 batches of test_gpu_lgcn_branch.batch (users with replacement, positives by Zipf; the
    last one for a closing loss-only step) -> dict, every array read-only"""
    from test_gpu_lgcn_branch import batch, lgcn_graph
    M, rs = lgcn_graph(7 * n_layers + d + asym, N_USERS, N_ITEMS, 4000, asym)
    Mt = M.T.tocsr()
    Mt.sort_indices()
    T0 = (rs.standard_normal((N_USERS + N_ITEMS, d)) * 0.1).astype(np.float32)
    w0, wu0 = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    batches = tuple(batch(rs, N_USERS, N_ITEMS, B) for _ in range(STEPS + 1))
    for a in (T0, w0, wu0) + tuple(x for b in batches for x in b):
        a.setflags(write=False)
    return dict(A=M, At=Mt if asym else None, T=T0, w=w0, wu=wu0, batches=batches)


@functools.lru_cache(maxsize=None)
def reference(kind, asym, n_layers, d, B):
    """the float64 trajectory of a problem, once: `losses` (STEPS + 1, 3) (the last row: the closing batch at the final
    parameters), final T, w, wu and the six slots.  One bpr_ref.Adam over [T, w, w_user]; bce steps T alone."""
    pr = problem(asym, n_layers, d, B)
    A64 = pr["A"].astype(np.float64)
    At64 = None if pr["At"] is None else pr["At"].astype(np.float64)
    both = kind == "bceboth"
    ref = Adam([pr["T"], pr["w"], pr["wu"]], LR)
    step = lambda u, i, j: lgcn_both(A64, ref.params[0], ref.params[1], ref.params[2], N_USERS, n_layers, u, i, j, ALPHA, BETA,
                                     DECAY, BS, both, At=At64)
    losses = []
    for u, i, j in pr["batches"][:STEPS]:
        out = step(u, i, j)
        losses.append(out[:3])
        ref.step(list(out[3:]) if both else [out[3]])      # (Adam.step zips: the vectors without a gradient are left out)
    losses.append(step(*pr["batches"][STEPS])[:3])
    out = dict(losses=np.asarray(losses), T=ref.params[0], w=ref.params[1], wu=ref.params[2], mT=ref.m[0], vT=ref.v[0],
               mw=ref.m[1], vw=ref.v[1], mwu=ref.m[2], vwu=ref.v[2])
    for a in out.values():
        a.setflags(write=False)
    return out


def used(got, want, name, steps=STEPS, lr=LR):
    """{label: worst difference / bound} of a final tensor under the tolerances of tests/test_gpu_lgcn_trajectory.py (a value
    above 1 misses its bound): T, w, wu: max |diff| <= 2e-3 lr steps and mean |diff| <= 1e-4 lr steps (test_twenty_step_trajectory,
    test_mf_twenty_step_trajectory_stays_on_the_oracle); a slot: |diff| <= 2e-4 |want| + 2e-6 max |want| element-wise (the MF
    trajectory test's slot tolerance)"""
    diff = np.abs(np.asarray(got, np.float64) - want)
    if name in ("T", "w", "wu"):
        return {name + " max": float(diff.max() / (2e-3 * lr * steps)), name + " mean": float(diff.mean() / (1e-4 * lr * steps))}
    atol = 2e-6 * np.abs(want).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff > 0, diff / (2e-4 * np.abs(want) + atol), 0.0)     # (a zero bound: a slot that must be exactly zero)
        # the share of the RELATIVE part in use once the absolute part is granted whole
        rel = np.where(diff > atol, (diff - atol) / (2e-4 * np.abs(want)), 0.0)
    return {name: float(r.max()), name + " rtol": float(rel.max())}
