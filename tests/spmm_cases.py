"""Shared inputs of the SpMM hub-reduction tests (tests/test_spmm_plan_cpu.py, tests/test_gpu_spmm_hubs.py,
tests/spmm_knob_worker.py): graphs whose hub rows reach every branch of the two-level piece reduction of
macr_amd/csrc/spmm_kernels.hip, a decoder of the plan buffer, and operands whose propagation is EXACT in fp32.

The exact-arithmetic method: weights are W * 2^-k with integer W, E0 is integer, so every product and every partial sum of
layer l is an integer multiple of the granule 2^-(k l).  While the sum of the |terms| of every row and every running layer
sum stay below 2^24 granules, each partial sum is representable in fp32 IN ANY SUMMATION ORDER: pieces, groups, half-waves
and fma chains all give the same bits, and they are the bits of an int64 computation.  One lost, doubled or mispaired entry
moves the result by at least one granule.
"""
import contextlib
import ctypes
import os

import numpy as np
import scipy.sparse as sp

K_GROUP = 16                # spmm_kernels.hip kGroup: pieces per group, groups per second-level round
REC_ENTRIES, REC_INTS = 32, 80
STREAM_PIECE = 256          # kStreamPiece: 255 neighbours + the end marker
PLAN_MAGIC, STREAM_MAGIC = 0x4d414356, 0x4d535452
PLAN_KNOBS = ("MACR_SPMM_CHUNK", "MACR_SPMM_OCTANTS", "MACR_SPMM_HUB", "MACR_SPMM_T", "MACR_SPMM_STREAM")


# ----------------------------------------------------------------------------- graphs
def hub_graph(n_users, n_items, hubs, seed=0):
    """0/1 pattern of the symmetrised bipartite graph [[0, R], [R^T, 0]] (CSR, sorted indices, float32 ones): every
    (item, degree) of `hubs` is linked to `degree` distinct random users, and every user to one random other item."""
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for item, degree in hubs:
        rows.append(rs.choice(n_users, degree, replace=False))
        cols.append(np.full(degree, item))
    others = np.setdiff1d(np.arange(n_items), [h for h, _ in hubs])
    rows.append(np.arange(n_users))
    cols.append(others[rs.randint(0, len(others), n_users)])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    R = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items)).tocsr()
    assert R.nnz == len(rows)                                   # no pair twice
    A = sp.bmat([[None, R], [R.T, None]]).tocsr().astype(np.float32)
    A.sort_indices()
    return A


def sym_norm(A):
    """D^-1/2 A D^-1/2 (--adj_type pre)"""
    deg = np.asarray(A.sum(1)).ravel()
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1)), 0.0)
    M = (sp.diags(dinv) @ A @ sp.diags(dinv)).tocsr().astype(np.float32)
    M.sort_indices()
    return M


def row_norm(A):
    """-> (D^-1 A, its transpose), both CSR (--adj_type norm / mean)"""
    deg = np.asarray(A.sum(1)).ravel()
    M = (sp.diags(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0)) @ A).tocsr().astype(np.float32)
    M.sort_indices()
    Mt = M.T.tocsr().astype(np.float32)
    Mt.sort_indices()
    return M, Mt


SMALL_SHAPE = (9000, 64)
SMALL_HUBS = [(0, 8192), (1, 8193), (2, 8704), (3, 513), (4, 9000)]
SMALL_SEED = 0
SMALL_GROUPS_OCTANTS = [16, 3, 16, 4, 16, 8, 8, 16, 8]     # pieces per group of the default row plan (tests/test_spmm_plan_cpu.py)
DEEP_SHAPE = (140000, 64)
DEEP_HUBS = [(0, 131073), (1, 70000)]
_cache = {}


def small():
    """N = 9 064, ~87 k non-zeros.  Row plan without octants: an exactly-full single group (8 192 = 16 pieces), rows of a full
    group + a group of ONE piece (8 193, 8 704), a two-piece hub (513), 16 + 2 (9 000); with octants every hub has two
    groups or eight short pieces.  The stream schedule cuts the same rows into 255-entry pieces: several groups per row."""
    if "small" not in _cache:
        _cache["small"] = hub_graph(SMALL_SHAPE[0], SMALL_SHAPE[1], SMALL_HUBS, SMALL_SEED)
    return _cache["small"]


def deep():
    """N = 140 064, ~682 k non-zeros; all 64 items are hub rows.  Item 0 (131 073 neighbours) has 17 groups in the row plan
    and 33 in the stream: the second-level loop runs more than one round of kGroup groups in both kernels."""
    if "deep" not in _cache:
        _cache["deep"] = hub_graph(DEEP_SHAPE[0], DEEP_SHAPE[1], DEEP_HUBS, 1)
    return _cache["deep"]


def sparse_graph():
    """1 900 x 517 with rows without neighbours and five hub items (the graph of
    test_lgcn_propagate_entry_stream_and_piece_orders), normalised D^-1/2 A D^-1/2"""
    if "sparse" not in _cache:
        rs = np.random.RandomState(17)
        n_users, n_items = 1900, 517
        R = (rs.rand(n_users, n_items) < 0.02).astype(np.float32)
        R[:, :5] = (rs.rand(n_users, 5) < 0.7)
        R[:3, :] = 0; R[:, 40:47] = 0
        A = sp.bmat([[None, sp.csr_matrix(R)], [sp.csr_matrix(R.T), None]]).tocsr().astype(np.float32)
        _cache["sparse"] = sym_norm(A)
    return _cache["sparse"]


def isolated():
    """600 users x 8 items (item 0 a hub of 600) followed by 20 000 rows without neighbours: N = 20 608.  The entry stream has
    a dozen chunks, so the rows without neighbours outnumber what its chunk descriptors can name (255 each): descriptors
    without entries take the rest."""
    if "isolated" not in _cache:
        A = hub_graph(600, 8, [(0, 600)], 2)
        n = 20000
        B = sp.bmat([[A, None], [None, sp.csr_matrix((n, n), dtype=np.float32)]]).tocsr().astype(np.float32)
        B.sort_indices()
        _cache["isolated"] = B
    return _cache["isolated"]


STAR_SHAPE = (640, 40)
STAR_HUB = 520


def star():
    """640 users x 40 items, N = 680: item 0 is linked to users 0..519 -- 520 entries, just above the 512 at which a plan
    splits a row -- and every user to one random other item.  Small enough for FOUR exact layers (exact_case: 520^3 weights
    of at most 3 stay below 2^24 granules; a fifth layer cannot with a hub this long)."""
    if "star" not in _cache:
        n_users, n_items = STAR_SHAPE
        rs = np.random.RandomState(3)
        rows = np.concatenate([np.arange(STAR_HUB), np.arange(n_users)])
        cols = np.concatenate([np.zeros(STAR_HUB, np.int64), 1 + rs.randint(0, n_items - 1, n_users)])
        R = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=STAR_SHAPE).tocsr()
        assert R.nnz == len(rows)
        A = sp.bmat([[None, R], [R.T, None]]).tocsr().astype(np.float32)
        A.sort_indices()
        _cache["star"] = A
    return _cache["star"]


# ----------------------------------------------------------------------------- plans
def build_plan_host(A, lib):
    """the plan of CSR matrix A as macr_spmm_plan_build writes it (int32 array), under the environment of the moment"""
    rowptr = np.ascontiguousarray(A.indptr, np.int32)
    col = np.ascontiguousarray(A.indices, np.int32)
    val = np.ascontiguousarray(A.data, np.float32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    N = len(rowptr) - 1
    nbytes = lib.macr_spmm_plan_bytes(N, hp(rowptr), hp(col), hp(val))
    assert nbytes > 0 and nbytes % 4 == 0
    host = np.zeros(nbytes // 4, np.int32)
    rc = lib.macr_spmm_plan_build(N, hp(rowptr), hp(col), hp(val), hp(host), host.nbytes)
    assert rc == 0, rc
    return host


def _groups(p, o, n_slots, n_groups, n_split):
    g = {}
    g["slot_group"] = p[o:o + n_slots]; o += n_slots
    g["group_slot0"] = p[o:o + n_groups + 1]; o += n_groups + 1
    g["group_split"] = p[o:o + n_groups]; o += n_groups
    g["split_group0"] = p[o:o + n_split + 1]; o += n_split + 1
    g["split_row"] = p[o:o + n_split]; o += n_split
    g["n_slots"], g["n_groups"], g["n_split"] = n_slots, n_groups, n_split
    return g, o


def decode_plan(plan_host):
    """Both schedules of a plan buffer as Python structures (layout comments of spmm_kernels.hip: PlanHeader / StreamHeader).
    -> dict: header fields, `items` (n_items, 4) = {row, beg, end, slot}, the group tables, `records` = list per class of
    (rows[R], cols[R, E], weights[R, E]) arrays, and `stream` (None without one) = header fields, `chunks` (n_chunks, 4),
    `empties`, the group tables, `pc` / `pw` (column word, weight word of every entry)."""
    p = np.asarray(plan_host, np.int32)
    names = ("magic", "n_items", "n_split", "n_slots", "N", "chunk", "n_groups", "reserved", "n_single", "rec_off")
    P = {n: int(p[k]) for k, n in enumerate(names)}
    P["n_rec"] = [int(x) for x in p[10:14]]
    assert P["magic"] == PLAN_MAGIC
    o = 16
    P["items"] = p[o:o + 4 * P["n_items"]].reshape(-1, 4); o += 4 * P["n_items"]
    g, o = _groups(p, o, P["n_slots"], P["n_groups"], P["n_split"])
    P.update(g)
    P["end_of_tables"] = o
    P["records"] = []
    if P["rec_off"] > 0:
        o = P["rec_off"]
        assert o == (P["end_of_tables"] + 3) // 4 * 4
        for c in range(4):
            R, E = 8 >> c, REC_ENTRIES // (8 >> c)
            rec = p[o:o + REC_INTS * P["n_rec"][c]].reshape(-1, REC_INTS); o += rec.size
            pairs = rec[:, 16:].reshape(-1, R, E, 2)
            P["records"].append((rec[:, :16], pairs[..., 0], pairs[..., 1].view(np.float32)))
        P["end_of_records"] = o
    P["stream"] = None
    if P["reserved"] > 0:
        o = P["reserved"]
        assert o % 16 == 0                                      # 64-byte aligned
        snames = ("magic", "n_chunks", "n_sb", "n_empty", "n_slots", "n_groups", "n_split", "n_entries")
        S = {n: int(p[o + k]) for k, n in enumerate(snames)}
        assert S["magic"] == STREAM_MAGIC
        o = (o + 8 + 3) // 4 * 4
        S["chunks"] = p[o:o + 4 * S["n_chunks"]].reshape(-1, 4); o += 4 * S["n_chunks"]
        S["empties"] = p[o:o + S["n_empty"]]; o += S["n_empty"]
        g, o = _groups(p, o, S["n_slots"], S["n_groups"], S["n_split"])
        S.update(g)
        o = (o + 15) // 16 * 16
        pcw = p[o:o + 2 * (S["n_entries"] + 128)].reshape(-1, 2); o += pcw.size
        assert o == len(p), (o, len(p))
        S["pc"], S["pw"] = pcw[:S["n_entries"], 0], pcw[:S["n_entries"], 1]
        S["tail"] = pcw[S["n_entries"]:]
        P["stream"] = S
    return P


def group_sizes(tables):
    """pieces per group, in group order (of the row plan or of the stream section)"""
    return [int(x) for x in np.diff(tables["group_slot0"])]


def groups_per_row(tables):
    """{hub row: number of groups}"""
    return {int(r): int(n) for r, n in zip(tables["split_row"], np.diff(tables["split_group0"]))}


# ----------------------------------------------------------------------------- exact operands
def exact_case(A_pattern, d, L, k=3, seed=0):
    """Operands whose L-layer propagation is exact in fp32 (see the module docstring) and its int64 result.
    -> dict: `A` (CSR fp32, the pattern with weights W 2^-k, W in {1, 2, 3}), `E0` (fp32, entries in {-1, 0, 1}), `want`
    (fp32: mean(E0, A E0, .., A^L E0), the exact sum rounded ONCE by the final multiplication with fp32(1 / (L + 1)), as
    the kernel's epilogue does), `terms_log2` / `sums_log2`: per layer, log2 of max_row sum |terms| and of max |running
    sum| in granules -- both asserted below 24."""
    Wi = A_pattern.copy().astype(np.int64)
    Wi.data = np.random.RandomState(seed).randint(1, 4, Wi.nnz).astype(np.int64)      # (the same matrix for every d and L)
    rs = np.random.RandomState(seed + 1 + 1000 * d + L)
    A = Wi.astype(np.float32)
    A.data = (Wi.data.astype(np.float64) * 2.0 ** -k).astype(np.float32)
    A.sort_indices()
    N = A.shape[0]
    X = rs.randint(-1, 2, (N, d)).astype(np.int64)
    E0 = X.astype(np.float32)
    S = X.copy()                                                # running sum, in granules of the current layer
    terms_log2, sums_log2 = [], []
    for l in range(1, L + 1):
        terms = Wi @ np.abs(X)                                  # sum of |w x| per row and column, granule 2^-(k l)
        X = Wi @ X
        S = S * (1 << k) + X
        terms_log2.append(float(np.log2(max(terms.max(), 1))))
        sums_log2.append(float(np.log2(max(np.abs(S).max(), 1))))
        assert terms.max() < 1 << 24, "layer %d: sum of |terms| = 2^%.1f granules" % (l, terms_log2[-1])
        assert np.abs(S).max() < 1 << 24, "layer %d: running sum = 2^%.1f granules" % (l, sums_log2[-1])
    total = (S.astype(np.float64) * 2.0 ** -(k * L)).astype(np.float32)
    assert np.array_equal(total.astype(np.float64) * 2.0 ** (k * L), S)      # (exact: |S| < 2^24)
    inv = np.float32(1.0) / np.float32(L + 1)
    want = (total * inv).astype(np.float32)                     # one fp32 rounding
    return dict(A=A, E0=E0, want=want, terms_log2=terms_log2, sums_log2=sums_log2)


# ----------------------------------------------------------------------------- device side (GPU tests and their worker)
@contextlib.contextmanager
def plan_env(env):
    """the plan-time knobs set to exactly `env` while a plan is built (they are read per plan build)"""
    saved = {k: os.environ.get(k) for k in PLAN_KNOBS}
    try:
        for k in PLAN_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_csr(ops, A, env):
    """A on the device with a plan built under the knobs `env`; env None: no plan (one wave per row)"""
    if env is None:
        return ops.CSR(dev(A.indptr.astype(np.int32)), dev(A.indices.astype(np.int32)), dev(A.data.astype(np.float32)))
    with plan_env(env):
        return ops.CSR.from_scipy(A, "cuda")


def assert_same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise AssertionError("%s: %d elements in %d rows differ, first at row %d column %d: got %r, want %r (rows: %s)" % (
            what, bad.sum(), bad.any(1).sum(), r, c, got[r, c], want[r, c], np.flatnonzero(bad.any(1))[:8]))


def run_exact(ops, case, adj, L, what, work=None, out=None):
    """one propagation of an exact case, compared bit for bit; -> the kernel names of the launches"""
    E0 = dev(case["E0"])
    if out is None:
        out = _torch().empty_like(E0)
    out.fill_(float("nan"))                                     # (a row nobody writes must not pass on what an earlier run left)
    ops.timing_begin()
    got = ops.lgcn_propagate(adj, E0, L, out=out, work=work).cpu().numpy()
    names = [n for n, _ in ops.timing_end(16)]
    assert len(names) == L, names
    assert_same_bits(got, case["want"], what)
    return names


def hub_batch(rs, n_users, n_items, B):
    """a batch on SMALL whose hub items are referred to >= 3 times (item 0), once (item 4) and never (item 2): the reference
    counts the hub finishers of the fused optimizer see"""
    pool = np.setdiff1d(np.arange(n_items), [2, 4])
    u = rs.choice(n_users, B, replace=False).astype(np.int32)
    i = pool[rs.randint(0, len(pool), B)].astype(np.int32)
    j = pool[rs.randint(0, len(pool), B)].astype(np.int32)
    i[:3] = 0
    i[3] = 4
    assert (i == 0).sum() >= 3 and (i == 4).sum() + (j == 4).sum() == 1 and not (i == 2).any() and not (j == 2).any()
    return u, i, j


def lgcn_counts(ops, state):
    """the per-row reference counts of an LGCNState's workspace (train_kernels.hip carve_lgcn_ws: behind E, dE, G and the
    propagation buffers)"""
    from macr_amd import _lib
    N, d = state.T.shape
    up = lambda n: (n + 255) // 256 * 256
    wf = _lib.lib().macr_lgcn_work_floats(N, d, state.adj._plan_ptrs()[1])
    if state.adj_t is not None:
        wf = max(wf, _lib.lib().macr_lgcn_work_floats(N, d, state.adj_t._plan_ptrs()[1]))
    off = 3 * up(N * d * 4) + up(wf * 4)
    return state.ws[off:off + 4 * N].view(_torch().int32)


def lgcn_scratch_regions(ops, state):
    """{name: tensor view} of every region of a default-mode LGCNState's workspace that train_kernels.hip carve_lgcn_ws (and
    launch_propagate for the inside of `work`) calls zero between steps:
        dE        (N, d) floats behind E: the gradient w.r.t. the propagated table (the fused epilogue clears the batch's rows,
                  the dense route clears all of it on return)
        cnt       N int32: references of the current batch per row (= lgcn_counts)
        emb_acc   2048 doubles (kEmbSlots): emb_loss partial sums, read and cleared by k_lgcn_finalize
        sbr       N floats: --loss bce2's branch scalar per ego row
        arrivals  int32 arrival counters of the hub groups and rows of the adjacency's plan: inside `work`, behind the
                  4 N d floats of the layer buffers and the slab rows (pieces + groups of whichever schedule of the plan has
                  more), to the end of macr_lgcn_work_floats; `arrivals_t` the same of adj_t's plan.  Absent without a plan.
    gw, the kBranchSlots partial rows of the branch-vector gradients, is NOT among them.  adam_block (k_lgcn_finalize /
    k_adam_dense) stores zeros over the partial rows of a segment it consumes, but only the segments of the step's kind
    exist: under bce1 / bce2 pair_bwd still adds a w_user half into every row (sums of dsu e_u, which vanish only because
    sig(su) = 1 makes dsu = 0 in its arithmetic) and nothing clears it.  The step does not rely on gw being clean either:
    block 0 of k_pair_fwd clears all of it before the step's pair_bwd adds."""
    from macr_amd import _lib
    torch = _torch()
    N, d = state.T.shape
    up = lambda n: (n + 255) // 256 * 256
    nd = up(N * d * 4)
    plans = [state.adj] + ([state.adj_t] if state.adj_t is not None else [])
    wf = max(_lib.lib().macr_lgcn_work_floats(N, d, a._plan_ptrs()[1]) for a in plans)
    ws = state.ws
    out = {"dE": ws[nd:nd + N * d * 4].view(torch.float32)}
    work = ws[3 * nd:3 * nd + wf * 4]
    for key, a in zip(("arrivals", "arrivals_t"), plans):
        if a.plan_host is None:
            continue
        P = decode_plan(a.plan_host)
        S = P["stream"] or P
        slab_rows = max(P["n_slots"] + P["n_groups"], S["n_slots"] + S["n_groups"])
        n_cnt = max(P["n_groups"] + P["n_split"], S["n_groups"] + S["n_split"]) + 64
        lo = (4 * N * d + slab_rows * d) * 4
        assert lo + n_cnt * 4 == _lib.lib().macr_lgcn_work_floats(N, d, a._plan_ptrs()[1]) * 4 <= work.numel()
        out[key] = work[lo:lo + n_cnt * 4].view(torch.int32)
    off = 3 * nd + up(wf * 4)
    out["cnt"] = ws[off:off + 4 * N].view(torch.int32)
    off += up(4 * N)
    out["emb_acc"] = ws[off:off + 2048 * 8].view(torch.float64)
    off += 2048 * 8
    out["sbr"] = ws[off:off + 4 * N].view(torch.float32)
    return out


def assert_scratch_clean(ops, state, what):
    """every region of lgcn_scratch_regions holds zeros (a NaN counts as dirt)"""
    for name, region in lgcn_scratch_regions(ops, state).items():
        dirty = int((region != 0).sum())
        assert dirty == 0, "%s: %d non-zero entries left in %s" % (what, dirty, name)


def _torch():
    import torch
    return torch


LR, DECAY, ALPHA, BETA = 1e-3, 1e-4, 1e-2, 1e-3


def run_train_case(ops, d, kind, env, asym=False, B=256, steps=3, L=2, twin=True):
    """Three training steps on SMALL (hub rows of two groups; with the row-normalised adjacency also in the plan of A^T):
      * against the CPU oracle with the tolerances of test_lgcn_train_step_matches_oracle (losses 1e-5 relative, first-step
        gradient through mT / 0.1, tables) -- LOSS_BPR_LGCN, which the oracle does not state, against the float64
        restatement tests/bpr_ref.py with the tolerances of test_lightgcn_bpr_steps;
      * against the same state stepped with dense_layers=True, as test_lgcn_batch_row_sparse_layers_equal_dense_layers;
      * the reference counts are all zero after every step.
    -> the kernel names of the last step's launches"""
    import oracle
    import bpr_ref
    n_users, n_items = SMALL_SHAPE
    N = n_users + n_items
    if asym:
        A, At = row_norm(small())
    else:
        A, At = sym_norm(small()), None
    rs = np.random.RandomState(100 + d + kind)
    T0 = (rs.standard_normal((N, d)) * 0.1).astype(np.float32)
    w0, wu0 = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    adj = device_csr(ops, A, env)
    adj_t = device_csr(ops, At, env) if asym else None
    for a in (adj, adj_t):
        if a is not None:
            assert max(groups_per_row(decode_plan(a.plan_host)).values()) >= 2       # hub rows beyond one group
    hyper = ops.make_hyper(LR, DECAY, ALPHA, BETA, B)
    mk = lambda: ops.LGCNState(dev(T0.copy()), n_users, n_items, dev(w0.copy()), dev(wu0.copy()), adj, L, hyper, B, adj_t=adj_t)
    state, dense = mk(), (mk() if twin else None)
    bpr = kind == ops.LOSS_BPR_LGCN
    if bpr:
        A64 = A.astype(np.float64)
        At64 = None if At is None else At.astype(np.float64)
        ref = bpr_ref.Adam([T0], LR)
    else:
        st = oracle.AdamState([T0.shape, (d,), (d,)])
        To, wo, wuo = T0.copy(), w0.copy(), wu0.copy()
        tr = None if At is None else (At.indptr, At.indices, At.data)
    names = []
    for t in range(steps):
        u, i, j = hub_batch(rs, n_users, n_items, B)
        if bpr:
            want = bpr_ref.lgcn_bpr(A64, ref.params[0], n_users, L, u, i, j, DECAY, B, At=At64)
            ref.step([want[3]])
            want, want_T, want_m = np.asarray(want[:3]), ref.params[0], ref.m[0]
        else:
            want = oracle.lgcn_train_step(kind, n_users, n_items, L, A.indptr, A.indices, A.data, u, i, j, To, wo, wuo, st,
                                          LR, DECAY, ALPHA, BETA, B, transposed=tr)
            want_T, want_m = To, st.m[0]
        ops.timing_begin()
        got = state.step(kind, dev(u), dev(i), dev(j)).cpu().numpy().copy()
        names = [n for n, _ in ops.timing_end(256)]
        assert not lgcn_counts(ops, state).any(), "step %d: reference counts left behind" % t
        Tg = state.T.cpu().numpy()
        if bpr:
            np.testing.assert_allclose(got, want, rtol=2e-5, err_msg="step %d" % t)
            diff = np.abs(Tg - want_T)
            assert diff.max() <= 2e-3 * LR * (t + 1) and diff.mean() <= 1e-4 * LR * (t + 1), (t, diff.max(), diff.mean())
            if t == 0:
                np.testing.assert_allclose(state.mT.cpu().numpy(), want_m, rtol=5e-4, atol=5e-6 * np.abs(want_m).max())
        else:
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg="step %d" % t)
            if t == 0:
                g_hip, g_orc = state.mT.cpu().numpy() / 0.1, want_m / 0.1
                np.testing.assert_allclose(g_hip, g_orc, rtol=5e-4, atol=2e-6 * np.abs(g_orc).max())
            np.testing.assert_allclose(Tg, want_T, rtol=0, atol=0.02 * LR * (t + 1))
        if dense is not None:
            lb = dense.step(kind, dev(u), dev(i), dev(j), dense_layers=True).cpu().numpy().copy()
            assert not lgcn_counts(ops, dense).any(), "step %d (dense layers): reference counts left behind" % t
            if t == 0:
                assert np.array_equal(got.view(np.uint32), lb.view(np.uint32))
                ga, gb = state.mT.cpu().numpy() / 0.1, dense.mT.cpu().numpy() / 0.1
                np.testing.assert_allclose(ga, gb, rtol=2e-5, atol=2e-7 * np.abs(gb).max())
            np.testing.assert_allclose(got, lb, rtol=2e-6)
            np.testing.assert_allclose(Tg, dense.T.cpu().numpy(), rtol=0, atol=2e-3 * LR * (t + 1))
    return names
