"""Batches that put the (B,B) loss kernel (k_bxb, macr_amd/csrc/train_kernels.hip) at the edges of its form choice, shared by
tests/test_bxb_cases_cpu.py (no GPU: the cases hold what they claim, and the oracle alone leaves room under the tolerances),
tests/test_gpu_bxb_forms.py (the kernel against the oracle) and tests/bxb_knob_worker.py (the same under MACR_BXB_ROWS /
MACR_BXB_NEUTRAL, which a process latches at its first launch).

What the launch decides, restated by classify():
  * pair_fwd flags column c when p[c] < -20 or n[c] > 6 or n[c] < -60;
  * a full batch (B % 256 == 0, neutral route on) takes the flagged columns of a 64-column tile with at most 8 of them out of
    the rotation (they rotate as (0, 0)) and evaluates them exactly in its neutral blocks;
  * a wave = (row group of 64 R rows, 64-column tile) takes the fast form iff for every column of its tile that is still in
    the rotation  p amax >= -20,  YLO <= n bmax <= 6  (YLO = -60 for R >= 2, -20 for R = 1)  and  amax, bmax <= 1, with
    amax / bmax the maxima of a / b over the group's real rows; pad rows and pad columns are zeros.

Every batch prescribes its row factors: ordinary rows have a, b <= 0.42, and a few CARRIER rows per row group hold the group's
amax = bmax = LEVEL_IN (0.5) in even groups and LEVEL_OUT (0.505) in odd ones.  An edge column aimed 0.5 % inside a threshold
at 0.5 (p = -39.8: p amax = -19.9) is therefore 0.5 % outside it in the odd groups (-20.1): the same columns give a fast wave
and an exact wave, on either side of the comparison, far beyond the ulps between the GPU's and the oracle's p and amax.
"""
import functools

import numpy as np

import oracle

D = 64
ALPHA, BETA, DECAY, BS = 1e-2, 1e-3, 1e-5, 1024          # as test_mf_train_step_matches_oracle
X_LO, Y_HI, Y_LO_PAIRS, Y_LO_SINGLE = -20.0, 6.0, -60.0, -20.0
NEUTRAL_TILE_MAX = 8
LEVEL_IN, LEVEL_OUT = 0.5, 0.505
SSU_CARRIER = 0.625                                      # sig(su) of a carrier row; its sig(si) = sig(sj) = level / 0.625


def default_rows(B):
    return 4 if B >= 4096 else 1


def _logit(x):
    return float(np.log(x / (1.0 - x)))


# ----------------------------------------------------------------------------------------------------------------- builder
def _aim(row, cons):
    """row (float64) + the minimum-norm correction after which row . v = t for the one or two (v, t) of cons"""
    if not cons:
        return row
    A = np.stack([v for v, _ in cons])
    r = np.asarray([t for _, t in cons]) - A @ row
    return row + A.T @ np.linalg.solve(A @ A.T, r)


def build_batch(B, targets, seed, d=D, scale=0.25):
    """targets: name -> (B,) float array, NaN where nothing is prescribed, for su = P[u].wu, si = Q[i].w, sj = Q[j].w,
    p = P[u].Q[i], n = P[u].Q[j].  -> u, i, j without a repeated row (each gradient row isolates one column), P, Q, w, wu.
    P[u] is corrected first (su), then Q[i] (si, p) and Q[j] (sj, n) against the corrected, rounded P[u]."""
    rs = np.random.RandomState(seed)
    n_users, n_items = 2 * B, 3 * B
    P = (rs.standard_normal((n_users, d)) * scale).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * scale).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    u = rs.choice(n_users, B, replace=False).astype(np.int32)
    ij = rs.choice(n_items, 2 * B, replace=False).astype(np.int32)
    i, j = ij[:B].copy(), ij[B:].copy()
    t = {k: np.asarray(targets.get(k, np.full(B, np.nan)), np.float64) for k in ("su", "si", "sj", "p", "n")}
    w64, wu64 = w.astype(np.float64), wu.astype(np.float64)
    for k in range(B):
        if not np.isnan(t["su"][k]):
            P[u[k]] = _aim(P[u[k]].astype(np.float64), [(wu64, t["su"][k])]).astype(np.float32)
    for rows, s_name, dot_name in ((i, "si", "p"), (j, "sj", "n")):
        for k in range(B):
            cons = []
            if not np.isnan(t[s_name][k]):
                cons.append((w64, t[s_name][k]))
            if not np.isnan(t[dot_name][k]):
                cons.append((P[u[k]].astype(np.float64), t[dot_name][k]))
            if cons:
                Q[rows[k]] = _aim(Q[rows[k]].astype(np.float64), cons).astype(np.float32)
    return u, i, j, P, Q, w, wu


# -------------------------------------------------------------------------------------------------------------- classifier
def row_factors(kind, si, sj, su):
    """a, b (fp32) as pair_fwd and the oracle form them from the branch logits"""
    one = np.float32(1.0)
    sig = lambda x: one / (one + np.exp(-np.asarray(x, np.float32)))
    ssu = sig(su) if kind == oracle.LOSS_RUBIBCEBOTH else np.ones(len(si), np.float32)
    return sig(si) * ssu, sig(sj) * ssu


def classify(p, n, a, b, B, R, full_neutral):
    """The launch's decisions from the fp32 forward scalars (oracle.pair_loss_grad's fwd; a, b: row_factors).
    -> dict: flags (B,) bool; count (tiles,) flagged columns per tile; neutral_tile (tiles,) bool; neutral (B,) bool: the
    columns taken out of the rotation; label (row groups, tiles) of "fast" / "exact"; xlo, yhi, ylo (row groups, tiles): the
    extremes of p amax and n bmax over the tile's columns in the rotation; amax, bmax (row groups,); real (row groups,): the
    group holds a real row."""
    f32 = np.float32
    p, n, a, b = (np.asarray(x, f32) for x in (p, n, a, b))
    Bp = (B + 255) // 256 * 256
    RB, nt = 64 * R, Bp // 64
    flags = (p < f32(-20.0)) | (n > f32(Y_HI)) | (n < f32(Y_LO_PAIRS))
    pad = lambda x: np.concatenate([x, np.zeros(Bp - B, x.dtype)])
    fl, pp, nn, aa, bb = pad(flags), pad(p), pad(n), pad(a), pad(b)
    count = fl.reshape(nt, 64).sum(1)
    neutral_tile = (count <= NEUTRAL_TILE_MAX) & (count > 0) & bool(full_neutral and B % 256 == 0)
    neutral = fl & np.repeat(neutral_tile, 64)
    pp, nn = np.where(neutral, f32(0), pp), np.where(neutral, f32(0), nn)
    amax = np.maximum(aa.reshape(-1, RB).max(1), f32(0))
    bmax = np.maximum(bb.reshape(-1, RB).max(1), f32(0))
    ylo_lim = f32(Y_LO_PAIRS if R >= 2 else Y_LO_SINGLE)
    xlo = (amax[:, None] * pp[None, :]).astype(f32)
    yv = (bmax[:, None] * nn[None, :]).astype(f32)
    out = ~(xlo >= f32(X_LO)) | ~(yv >= ylo_lim) | ~(yv <= f32(Y_HI)) | ~(amax <= 1)[:, None] | ~(bmax <= 1)[:, None]
    g = len(amax)
    exact = out.reshape(g, nt, 64).any(2)
    return dict(flags=flags, count=count, neutral_tile=neutral_tile, neutral=neutral[:B],
                label=np.where(exact, "exact", "fast"), xlo=xlo.reshape(g, nt, 64).min(2), yhi=yv.reshape(g, nt, 64).max(2),
                ylo=yv.reshape(g, nt, 64).min(2), amax=amax, bmax=bmax, real=np.arange(g) * RB < B)


# --------------------------------------------------------------------------------------------------- float64 restatement
def f64_reference(kind, u, i, j, P, Q, w, wu, alpha=ALPHA, beta=BETA, decay=DECAY, bs=BS, block=128):
    """The loss graph of rubibceboth / rubibce (the reference's model.py:185-222 / :158-183, the expression of
    orc_pair_loss_grad) in float64 on the fp32 tables, the (B,B) term in blocks of rows:
        X[r,c] = p[c] a[r],  Y[r,c] = n[c] b[r],  L_ori = mean(-log(sig(X) + 1e-10) - log(1 - sig(Y) + 1e-10)),
    with 1 - sig(Y) formed as sig(-Y).  -> losses, dp, dn, da, db, the per-column share col_l of L_ori (they sum to it), the
    derivatives dsi, dsj, dsu by the branch logits, and the gradients of the gathered rows and branch vectors with the regulariser's part."""
    f = lambda x: np.asarray(x, np.float64)
    eu, ei, ej, w, wu = f(P[u]), f(Q[i]), f(Q[j]), f(w), f(wu)
    B = len(u)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    eps = 1e-10
    p, n = (eu * ei).sum(1), (eu * ej).sum(1)
    si, sj, su = ei @ w, ej @ w, eu @ wu
    both = kind == oracle.LOSS_RUBIBCEBOTH
    ssi, ssj, osj = sig(si), sig(sj), sig(-sj)
    ssu, osu = (sig(su), sig(-su)) if both else (np.ones(B), np.zeros(B))
    a, b = ssi * ssu, ssj * ssu
    dp, dn, da, db, col_l = (np.zeros(B) for _ in range(5))
    for r0 in range(0, B, block):
        ar, br = a[r0:r0 + block, None], b[r0:r0 + block, None]
        X, Y = ar * p[None, :], br * n[None, :]
        sx, ox, sy, oy = sig(X), sig(-X), sig(Y), sig(-Y)
        col_l += (-np.log(sx + eps) - np.log(oy + eps)).sum(0)
        fx, gy = -(sx * ox) / (sx + eps), (sy * oy) / (oy + eps)
        dp += (fx * ar).sum(0)
        dn += (gy * br).sum(0)
        da[r0:r0 + block] = (fx * p[None, :]).sum(1)
        db[r0:r0 + block] = (gy * n[None, :]).sum(1)
    b2 = float(B) * float(B)
    dp, dn, da, db, col_l = dp / b2, dn / b2, da / b2, db / b2, col_l / b2
    l_ori = col_l.sum()
    l_item = (-np.log(ssi + eps) - np.log(osj + eps)).mean()
    l_user = (-np.log(ssu + eps) - np.log(osu + eps)).mean() if both else 0.0
    mf = l_ori + alpha * l_item + (beta * l_user if both else 0.0)
    reg = decay * 0.5 * ((eu * eu).sum() + (ei * ei).sum() + (ej * ej).sum()) / bs
    dsi = da * ssi * (1 - ssi) * ssu + (alpha / B) * -(ssi * (1 - ssi)) / (ssi + eps)
    dsj = db * ssj * osj * ssu + (alpha / B) * (ssj * osj) / (osj + eps)
    dsu = ((da * ssi + db * ssj) * ssu * osu + (beta / B) * (-(ssu * osu) / (ssu + eps) + (ssu * osu) / (osu + eps))) if both \
        else np.zeros(B)
    coef = decay / bs
    deu = dp[:, None] * ei + dn[:, None] * ej + dsu[:, None] * wu[None, :] + coef * eu
    dei = dp[:, None] * eu + dsi[:, None] * w[None, :] + coef * ei
    dej = dn[:, None] * eu + dsj[:, None] * w[None, :] + coef * ej
    dw = (ei * dsi[:, None]).sum(0) + (ej * dsj[:, None]).sum(0)
    dwu = (eu * dsu[:, None]).sum(0)
    return dict(l_ori=l_ori, l_item=l_item, l_user=l_user, mf=mf, reg=reg, loss=mf + reg, col_l=col_l, dp=dp, dn=dn, da=da,
                db=db, dsi=dsi, dsj=dsj, dsu=dsu, deu=deu, dei=dei, dej=dej, dw=dw, dwu=dwu)


# ------------------------------------------------------------------------------------------------------------------- cases
def _edge_values(ylo):
    """column targets (p, n) by name: *_in lies 0.5 % inside its threshold at LEVEL_IN (and 0.5 % outside it at LEVEL_OUT),
    *_out 0.5 % outside at LEVEL_IN, *_far well outside whatever the row.  Columns aimed at very negative n carry p = -15:
    with both terms vanishing a column would weigh nothing in L_ori (and x >= 15 with y <= -59 is where the fp32 reference
    itself is 13 % off its term)."""
    nan = np.nan
    return {"x_in": (X_LO * 0.995 / LEVEL_IN, nan), "x_out": (X_LO * 1.005 / LEVEL_IN, nan),
            "yhi_in": (nan, Y_HI * 0.995 / LEVEL_IN), "yhi_out": (nan, Y_HI * 1.005 / LEVEL_IN),
            "ylo_in": (-15.0, ylo * 0.995 / LEVEL_IN), "ylo_out": (-15.0, ylo * 1.005 / LEVEL_IN),
            "p_far": (-45.0, nan), "n_hi_far": (nan, 25.0), "n_lo_far": (-15.0, -70.0)}


def _row_targets(rs, B, R, kind, a1):
    """si, sj, su of every row and the carrier rows: ordinary rows sig(si), sig(sj) in [0.2, 0.7], sig(su) in [0.3, 0.6]; three
    carriers per group of 64 R rows (fewer in a short last group) at the group's level.  a1 (rubibce): the carriers have
    si = 20, so sig(si) == 1.0f == a, and sig(sj) = 0.8."""
    si = np.array([_logit(x) for x in rs.uniform(0.2, 0.7, B)])
    sj = np.array([_logit(x) for x in rs.uniform(0.2, 0.7, B)])
    su = np.array([_logit(x) for x in rs.uniform(0.3, 0.6, B)])
    RB, carriers = 64 * R, []
    for g in range((B + RB - 1) // RB):
        real = min(RB, B - g * RB)
        level = LEVEL_IN if g % 2 == 0 else LEVEL_OUT
        for off in sorted({1 % real, real // 2, real - 1}):
            r = g * RB + off
            carriers.append(r)
            if a1:
                si[r], sj[r] = 20.0, _logit(0.8)
            else:
                si[r] = sj[r] = _logit(level / SSU_CARRIER)
                su[r] = _logit(SSU_CARRIER)
    return si, sj, su, carriers


def _partial_columns(B, ylo):
    """tile 0 / 1 / 2: columns just inside the p, the upper n and the lower n threshold (fast in even row groups, exact in
    odd ones); tile 3: one column just outside in p (exact in every group); the last, partial tile: one just outside the upper
    n threshold.  With more tiles (B = 4100) the same again further out, the lower n threshold's outside included."""
    cols = {5: "x_in", 40: "x_in", 64 + 7: "yhi_in", 64 + 50: "yhi_in", 128: "ylo_in", 128 + 63: "ylo_in", 192 + 20: "x_out",
            B - 2: "yhi_out"}
    expect = {"in_tiles": [0, 1, 2], "out_tiles": [3, (B - 1) // 64]}
    if B >= 4096:
        cols.update({640 + 33: "x_in", 704 + 1: "yhi_in", 768 + 62: "ylo_in", 1280 + 9: "yhi_out", 1920 + 17: "ylo_out",
                     2560 + 31: "x_out", 3840 + 63: "ylo_out"})
        expect["in_tiles"] += [10, 11, 12]
        expect["out_tiles"] += [20, 30, 40, 60]
    return cols, expect


def _full_columns(B, R, ylo):
    """tile 0: flags at positions 0 and 63; tile 1: 8 flags inside columns 64..79 (one lane of the neutral block's scan);
    tile 3: 8 flags, 2 per 16-column quarter; tile 5: 9 flags, every one just INSIDE the window at LEVEL_IN (flagged by column,
    fast by the wave's test in even row groups); tile 7 (B > 512): 9 flags, one of them just outside (exact everywhere);
    tile 17 (B > 1024): 8 flags, positions 0 and 63 among them, in the second trip of the scan."""
    far = ["p_far", "n_hi_far", "n_lo_far", "x_out", "yhi_out", "p_far", "n_hi_far", "n_lo_far"]
    ins = ["x_in", "yhi_in"] + (["ylo_in"] if R >= 2 else [])              # flagged AND inside the wave's window at LEVEL_IN
    cols = {0: "n_hi_far", 63: "n_lo_far"}
    for k, pos in enumerate([0, 1, 3, 4, 7, 9, 12, 15]):
        cols[64 + pos] = far[k]
    for k, pos in enumerate([2, 13, 16, 31, 40, 47, 48, 63]):
        cols[192 + pos] = far[(k + 3) % 8]
    for k, pos in enumerate([0, 5, 11, 22, 30, 37, 44, 58, 63]):
        cols[320 + pos] = ins[k % len(ins)]
    count = {0: 2, 1: 8, 3: 8, 5: 9}
    expect = {"flagged_fast_tile": 5, "lane_tile": 1, "spread_tile": 3}
    if B > 512:
        for k, pos in enumerate([1, 8, 15, 16, 29, 33, 46, 50, 62]):
            cols[448 + pos] = "x_out" if k == 4 else ins[k % len(ins)]
        count[7] = 9
        expect["nine_exact_tile"] = 7
    if B > 1024:
        for k, pos in enumerate([0, 10, 20, 27, 35, 49, 55, 63]):
            cols[1088 + pos] = far[(k + 1) % 8]
        count[17] = 8
        expect["second_trip_tile"] = 17
    expect["count"] = count
    return cols, expect


def _a1_columns():
    """rubibce with a == 1.0f carriers: tile 1: raw p = -19.9, unflagged and inside the window at amax = 1 exactly; tile 4:
    p = -20.1 twice, flagged and neutralised; tile 6: p = -20.1 nine times, flagged and left to an exact wave."""
    cols = {64 + 3: -19.9, 64 + 30: -19.9, 64 + 63: -19.9, 256 + 0: -20.1, 256 + 41: -20.1}
    for pos in [0, 6, 13, 21, 28, 36, 45, 52, 63]:
        cols[384 + pos] = -20.1
    return cols, {"count": {4: 2, 6: 9}, "a1_tile": 1, "neutral_a1_tile": 4, "nine_exact_tile": 6}


# name -> B, R the launch will use, loss kind, layout, and what a worker process must find in its environment
CASES = {
    "partial_r1": dict(B=300, R=1, layout="partial"),
    "partial_r4": dict(B=4100, R=4, layout="partial"),
    "full_r1": dict(B=1280, R=1, layout="full"),
    "full_r4": dict(B=4096, R=4, layout="full"),
    "item_branch_a1": dict(B=512, R=1, layout="a1", kind=oracle.LOSS_RUBIBCE),
    "rows2_partial": dict(B=300, R=2, layout="partial", env={"MACR_BXB_ROWS": "2"}),
    "rows2_full": dict(B=512, R=2, layout="full", env={"MACR_BXB_ROWS": "2"}),
    "rows4_partial": dict(B=300, R=4, layout="partial", env={"MACR_BXB_ROWS": "4"}),
    "rows4_full": dict(B=512, R=4, layout="full", env={"MACR_BXB_ROWS": "4"}),
    "neutral_off": dict(B=512, R=1, layout="full", neutral=False, env={"MACR_BXB_NEUTRAL": "0"}),
    "neutral_on": dict(B=512, R=1, layout="full"),          # neutral_off's batch under the default launch
}
IN_PROCESS = ["partial_r1", "partial_r4", "full_r1", "full_r4", "item_branch_a1"]
WORKER_SETTINGS = {"rows2": ["rows2_partial", "rows2_full"], "rows4": ["rows4_partial", "rows4_full"], "neutral0": ["neutral_off"]}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the batch (u, i, j, P, Q, w, wu; do not modify), kind, B, R, neutral (the launch has neutral blocks), cols
    (column -> name or raw p of every edge column), carriers, expect (what test_bxb_cases_cpu.py holds classify() to)"""
    spec = CASES[name]
    B, R, layout = spec["B"], spec["R"], spec["layout"]
    kind = spec.get("kind", oracle.LOSS_RUBIBCEBOTH)
    ylo = Y_LO_PAIRS if R >= 2 else Y_LO_SINGLE
    seed = 1000 * R + B + {"partial": 1, "full": 2, "a1": 3}[layout]
    rs = np.random.RandomState(seed)
    si, sj, su, carriers = _row_targets(rs, B, R, kind, layout == "a1")
    p, n = np.full(B, np.nan), np.full(B, np.nan)
    if layout == "a1":
        cols, expect = _a1_columns()
        for c, v in cols.items():
            p[c] = v
    else:
        cols, expect = _partial_columns(B, ylo) if layout == "partial" else _full_columns(B, R, ylo)
        ev = _edge_values(ylo)
        for c, v in cols.items():
            p[c], n[c] = ev[v]
    u, i, j, P, Q, w, wu = build_batch(B, dict(su=su, si=si, sj=sj, p=p, n=n), seed)
    return dict(name=name, B=B, R=R, kind=kind, layout=layout, neutral=spec.get("neutral", True) and B % 256 == 0,
                env=spec.get("env", {}), u=u, i=i, j=j, P=P, Q=Q, w=w, wu=wu, cols=cols, carriers=carriers, expect=expect)


def oracle_forward(c):
    """one pass of the oracle's loss graph over the case's batch (no step): its dict + p, n, a, b and classify()'s verdict"""
    o = oracle.pair_loss_grad(c["kind"], c["P"][c["u"]], c["Q"][c["i"]], c["Q"][c["j"]], c["w"], c["wu"], ALPHA, BETA)
    p, n, si, sj, su = o["fwd"]
    a, b = row_factors(c["kind"], si, sj, su)
    o.update(p=p, n=n, a=a, b=b, cls=classify(p, n, a, b, c["B"], c["R"], c["neutral"]))
    return o


def label_counts(cls):
    """what a summary lists: waves with a real row by label, flagged columns, tiles by flag count, neutralised columns"""
    lab = cls["label"][cls["real"]]
    counts = {int(k): int(v) for k, v in zip(*np.unique(cls["count"][cls["count"] > 0], return_counts=True))}
    return dict(fast=int((lab == "fast").sum()), exact=int((lab == "exact").sum()), flagged=int(cls["flags"].sum()),
                tiles_by_flag_count=counts, neutralised=int(cls["neutral"].sum()))


# -------------------------------------------------------------------------------------------------------------- on the GPU
@functools.lru_cache(maxsize=None)
def oracle_two_steps(name, lr=1e-4):
    """the oracle's two steps on the case's batch at lr: losses of both and the Adam first moments after the first (0.1 x the
    gradient; neither they nor the first step's losses depend on lr)"""
    c = case(name)
    P, Q, w, wu = c["P"].copy(), c["Q"].copy(), c["w"].copy(), c["wu"].copy()
    st = oracle.AdamState([P.shape, Q.shape, (D,), (D,)])
    first = oracle.mf_train_step(c["kind"], c["u"], c["i"], c["j"], P, Q, w, wu, st, lr, DECAY, ALPHA, BETA, BS).copy()
    m = [x.copy() for x in st.m]
    second = oracle.mf_train_step(c["kind"], c["u"], c["i"], c["j"], P, Q, w, wu, st, lr, DECAY, ALPHA, BETA, BS).copy()
    return first, second, m


def run_on_gpu(ops, name, note=print):
    """The case on the GPU against the oracle; raises AssertionError, -> the measured distances and the complete step's losses.
      * one complete step (lr 1e-3): losses 1e-5 relative; first-step gradients of P, Q, w, wu through m / 0.1 with the bounds
        of test_mf_rubibceboth_large_logits (rtol 5e-4, atol 2e-6 max); everything finite; gradient scratch and flags zero;
      * a twin taking the batch twice with defer=True at lr 1e-4, then flush(): the second call runs the (B,B) kernel's
        instantiation with the pending dense Adam pass on the same edges; both losses 1e-5 from the oracle's two steps."""
    import torch
    c = case(name)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    first, second, m = oracle_two_steps(name)
    kind, B = c["kind"], c["B"]
    batch = [dev(c[k]) for k in ("u", "i", "j")]
    res = {}
    state = ops.MFState(dev(c["P"]), dev(c["Q"]), dev(c["w"]), dev(c["wu"]), ops.make_hyper(1e-3, DECAY, ALPHA, BETA, BS), B)
    got = state.step(kind, *batch).cpu().numpy().copy()
    res["losses"] = [float(x) for x in got]
    res["loss_rel"] = float(np.max(np.abs(got.astype(np.float64) - first) / np.abs(first)))
    note("%s: complete step: gpu %r oracle %r max rel %.3e" % (name, got.tolist(), first.tolist(), res["loss_rel"]))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, first, rtol=1e-5, atol=0, err_msg=name)
    for gname, gm, om in (("P", state.mP, m[0]), ("Q", state.mQ, m[1]), ("w", state.mw, m[2]), ("wu", state.mwu, m[3])):
        g_hip, g_orc = gm.cpu().numpy() / 0.1, om / 0.1
        assert np.isfinite(g_hip).all(), gname
        scale = float(np.abs(g_orc).max())
        res["grad_%s" % gname] = float(np.max(np.abs(g_hip.astype(np.float64) - g_orc) / (5e-4 * np.abs(g_orc.astype(np.float64)) + 2e-6 * scale + 1e-300)))
        note("%s: d%s: worst |gpu - oracle| / bound = %.3f (max |g| %.3e)" % (name, gname, res["grad_%s" % gname], scale))
        np.testing.assert_allclose(g_hip, g_orc, rtol=5e-4, atol=2e-6 * scale, err_msg="%s d%s" % (name, gname))
    for tname in ("P", "Q", "w", "wu", "vP", "vQ", "vw", "vwu"):
        assert bool(torch.isfinite(getattr(state, tname)).all()), tname
    assert float(state.gP.abs().max()) == 0.0 and float(state.gQ.abs().max()) == 0.0
    assert int(state.tP.sum()) == 0 and int(state.tQ.sum()) == 0
    twin = ops.MFState(dev(c["P"]), dev(c["Q"]), dev(c["w"]), dev(c["wu"]), ops.make_hyper(1e-4, DECAY, ALPHA, BETA, BS), B,
                       lazy_period=1)
    t1 = twin.step(kind, *batch, defer=True).cpu().numpy().copy()
    t2 = twin.step(kind, *batch, defer=True).cpu().numpy().copy()
    assert twin.pending_B == B
    twin.flush()
    res["deferred_rel"] = [float(np.max(np.abs(t.astype(np.float64) - wnt) / np.abs(wnt))) for t, wnt in ((t1, first), (t2, second))]
    note("%s: deferred twin: gpu %r %r oracle %r %r max rel %r" % (name, t1.tolist(), t2.tolist(), first.tolist(), second.tolist(),
                                                                  res["deferred_rel"]))
    np.testing.assert_allclose(t1, first, rtol=1e-5, atol=0, err_msg=name + " deferred, first call")
    np.testing.assert_allclose(t2, second, rtol=1e-5, atol=0, err_msg=name + " deferred, second call")
    for tname in ("P", "Q", "w", "wu", "mP", "mQ", "vP", "vQ"):
        assert bool(torch.isfinite(getattr(twin, tname)).all()), tname
    assert float(twin.gP.abs().max()) == 0.0 and float(twin.gQ.abs().max()) == 0.0
    assert int(twin.tP.sum()) == 0 and int(twin.tQ.sum()) == 0
    return res
