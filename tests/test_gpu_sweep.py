"""The shared-listing-pass c sweep (macr_score_topk_sweep, the path of both tuners through Evaluator.sweep_means) against
the CPU oracle (-m gpu).

Every ranking assertion compares one (1,U,K) slice of the sweep's output, after macr_topk_merge, with oracle.score_topk called
for that value of c on the SAME sig_u / sig_i arrays (the HIP branch_sigmoid outputs, or hand-set fp32 values in (0,1)): item
ids, candidate counts and score BITS are equal -- no tolerance anywhere -- under each of the three candidate filters (the
sweep has bf16 kernels only and runs them under "f16").  The inputs and the oracle's lists of a case are computed once and
shared by the three filters; nothing modifies them.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle
from test_gpu_ops import random_mask, sampled_items

pytestmark = pytest.mark.gpu

RUBI_BOTH, RUBI, DIRECT_MINUS, DIRECT_MINUS_BOTH = (oracle.SCORE_RUBI_BOTH, oracle.SCORE_RUBI, oracle.SCORE_DIRECT_MINUS,
                                                    oracle.SCORE_DIRECT_MINUS_BOTH)
BOTH = (RUBI_BOTH, DIRECT_MINUS_BOTH)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


@pytest.fixture(params=["f32", "bf16", "f16"])
def eval_filter(request, ops, monkeypatch):
    """run the test once per candidate filter of the listing pass (include/macr_hip.h MACR_EVAL_FILTER_*): the ranking
    must be the fp32 ranking bit for bit either way"""
    monkeypatch.setenv("MACR_EVAL_FILTER", request.param)       # what an Evaluator created by the test picks up
    ops.set_eval_filter(request.param)
    yield request.param
    ops.set_eval_filter("env")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ----------------------------------------------------------------------------- problems and their oracle lists
class Problem(object):
    """The numpy side of one case: tables, query ids, branch factors, mask, and the oracle's lists per value of c (computed on
    first use, then shared).  sig_u is None for the kinds that do not read it: the sweep then gets a NULL pointer."""

    def __init__(self, kind, P, user_ids, Q, K, sig_u, sig_i, mask_lists):
        self.kind, self.P, self.user_ids, self.Q, self.K = kind, P, user_ids, Q, K
        self.sig_u = sig_u if kind in BOTH else None
        self.sig_i = sig_i
        assert sig_i.dtype == np.float32 and np.all(sig_i > 0) and np.all(sig_i < 1)
        self.mask_lists = mask_lists
        self.mask_csr = oracle.csr_from_lists(mask_lists) if mask_lists is not None else None
        self.U = P.shape[0] if user_ids is None else len(user_ids)
        self.N, self.d = Q.shape
        self._want = {}

    def rows(self):
        return self.P if self.user_ids is None else self.P[self.user_ids]

    def want(self, c):
        """(val, idx, cnt) of oracle.score_topk for this value of c on the whole catalogue"""
        c = float(np.float32(c))
        if c not in self._want:
            self._want[c] = oracle.score_topk(self.kind, self.rows(), self.Q, self.K, self.sig_u, self.sig_i, c, self.mask_csr, 0)
        return self._want[c]

    def mask_dev(self, ops):
        if self.mask_lists is None:
            return None
        mptr, midx = self.mask_csr
        return ops.CSR(dev(mptr), dev(midx if len(midx) else np.zeros(1, np.int32)))


def hip_sigmoids(ops):
    """(rows, w, ids) -> fp32 numpy: the HIP branch factors, which then feed both rankers"""
    def f(rows, w, ids=None):
        return ops.branch_sigmoid(dev(rows), dev(w), dev(ids)).cpu().numpy()
    return f


def run_sweep(ops, p, cs, lo=0, hi=None, mask=None):
    """the sweep on item rows [lo, hi) of the problem's catalogue -> (vals, idx) of shape (len(cs), U, K), global ids"""
    hi = p.N if hi is None else hi
    return ops.score_topk_sweep(p.kind, dev(p.P), dev(p.user_ids), dev(p.Q[lo:hi]), p.K, dev(p.sig_u), dev(p.sig_i[lo:hi]),
                                dev(np.asarray(cs, np.float32)), mask if mask is not None else p.mask_dev(ops), lo)


def assert_is_oracle(ops, p, vals, idx, c, tag):
    """one (W,U,K) stack of lists of one value of c, merged, is the oracle's ranking: ids, counts, score bits"""
    gv, gi, gc = ops.topk_merge(vals.contiguous(), idx.contiguous())
    wv, wi, wc = p.want(c)
    assert np.array_equal(gi.cpu().numpy(), wi), tag
    assert np.array_equal(gc.cpu().numpy(), wc), tag
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), wv.view(np.uint32)), tag          # bit for bit


def assert_sweep_is_oracle(ops, p, vals, idx, cs, tag):
    assert vals.shape == (len(cs), p.U, p.K) and idx.shape == vals.shape
    for g, c in enumerate(cs):
        assert_is_oracle(ops, p, vals[g:g + 1], idx[g:g + 1], c, (tag, g, c))


_CASES = {}


def shared(key, make):
    """the Problem of a case: built by the first filter that asks, the same object for the others"""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ----------------------------------------------------------------------------- 1. shape and kind matrix
# id: (d, kind, N, U, K, mean mask length or None, heavy, user_ids given, values of c, duplicated item rows)
# N: 5 and 33 around the 32-item tile, 257 one item past the 8-tile sampling window, 1024 the largest catalogue that lists
# everything, 1025 the smallest that samples, 2500 and 8993 several windows with a ragged last tile.  U: 1, 33, 257 (one query
# past a block of 256), 700.  n_c 1..4 at every d at least once; d = 256 with four values asks for the largest LDS budget.
MATRIX = {
    "d32-rubi-N5-U1-K1": (32, RUBI, 5, 1, 1, None, False, False, [0.0], False),
    "d64-dm-N33-U33-K20-unsorted": (64, DIRECT_MINUS, 33, 33, 20, 3, False, True, [40.0, -3.0], False),
    "d128-rubiboth-N1024-U257-K32-heavy": (128, RUBI_BOTH, 1024, 257, 32, 12, True, True, [0.0, 1e4, -2.5], True),
    "d256-dmboth-N1025-U33-K20": (256, DIRECT_MINUS_BOTH, 1025, 33, 20, None, False, False, [-3.0, 0.0, 12.5, 40.0], True),
    "d64-rubiboth-N2500-U700-K20-heavy-twice": (64, RUBI_BOTH, 2500, 700, 20, 12, True, True, [40.0, 0.0, 40.0, -3.0], True),
    "d256-rubi-N8993-U257-K32": (256, RUBI, 8993, 257, 32, 40, False, False, [1e4, -1e4, 0.0], True),
    "d32-dmboth-N8993-U700-K1": (32, DIRECT_MINUS_BOTH, 8993, 700, 1, 12, False, True, [1e4, 0.0], True),
    "d128-dm-N2500-U257-K32-nomask": (128, DIRECT_MINUS, 2500, 257, 32, None, False, False, [-40.0], True),
    "d64-rubi-N1024-U1-K20": (64, RUBI, 1024, 1, 20, 30, False, True, [12.5, -3.0, 0.0], True),
    "d32-rubiboth-N257-U33-K32-heavy": (32, RUBI_BOTH, 257, 33, 32, 6, True, False, [-3.0, 0.0, 40.0, 1e4], True),
    "d128-rubi-N1025-U700-K20-twice": (128, RUBI, 1025, 700, 20, 3, False, True, [0.5, 40.0, 0.5, -1e4], True),
    "d256-rubiboth-N5-U257-K20": (256, RUBI_BOTH, 5, 257, 20, None, False, True, [40.0, -3.0], False),
    "d64-dm-N8993-U33-K32-c1e4": (64, DIRECT_MINUS, 8993, 33, 32, 12, False, False, [0.0, 1e4, -3.0, 40.0], True),
}


def matrix_problem(name, sigmoid):
    d, kind, N, U, K, mean_len, heavy, with_ids, cs, dup = MATRIX[name]
    rs = np.random.RandomState(sorted(MATRIX).index(name) + 4000)
    n_users = U + 23 if with_ids else U
    P = (rs.standard_normal((n_users, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    Q += (rs.standard_normal(N).astype(np.float32) * 0.5)[:, None] * np.sign(P.mean(0, keepdims=True))   # popularity
    if dup:
        Q[N // 2:N // 2 + 10] = Q[:10]                           # exact ties far apart (equal rows, equal branch factors)
    w = (rs.standard_normal(d) * 0.3).astype(np.float32)
    wu = (rs.standard_normal(d) * 0.3).astype(np.float32)
    user_ids = rs.permutation(n_users)[:U].astype(np.int32) if with_ids else None
    mask = None
    if mean_len is not None:
        mask = random_mask(rs, U, N, mean_len, heavy=(0, U - 1) if heavy else ())
    return Problem(kind, P, user_ids, Q, K, sigmoid(P, wu, user_ids), sigmoid(Q, w), mask)


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_sweep_matrix_is_the_oracle_per_value(ops, name, eval_filter):
    """Every width, every number of values, the four kinds that read c, catalogues around the tile / the sampling window /
    the list-everything limit, K = 1, 20, 32, with and without a mask and query ids, three rows with queries that keep 4
    candidates (< K), c negative, 0, 40 and 1e4, unsorted sets, and sets that hold one value twice (the two slices are then
    equal to each other as well)."""
    cs = MATRIX[name][8]
    p = shared(("matrix", name), lambda: matrix_problem(name, hip_sigmoids(ops)))
    vals, idx = run_sweep(ops, p, cs)
    assert_sweep_is_oracle(ops, p, vals, idx, cs, name)
    for a in range(len(cs)):
        for b in range(a + 1, len(cs)):
            if cs[a] == cs[b]:
                assert torch.equal(idx[a], idx[b]) and torch.equal(vals[a].view(torch.int32), vals[b].view(torch.int32)), (name, a, b)


# ----------------------------------------------------------------------------- 2. item shards
def shard_problem(sigmoid):
    rs = np.random.RandomState(4100)
    U, N, d, K = 300, 5003, 64, 20
    P = (rs.standard_normal((U, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    Q[100:200] = Q[3300:3400]                                    # exact score ties across the shards of either split
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    return Problem(RUBI_BOTH, P, None, Q, K, sigmoid(P, wu), sigmoid(Q, w), random_mask(rs, U, N, 20, heavy=(7,)))


SHARD_CS = [-3.0, 12.5, 40.0]


@pytest.mark.parametrize("W", [2, 3])
def test_sweep_on_item_shards_merges_to_the_whole_catalogue(ops, W, eval_filter):
    """The sweep on W contiguous shards with item_offset = the shard's first id (mask ids stay global), merged per value with
    macr_topk_merge, is the oracle's ranking of the whole catalogue."""
    p = shared("shards", lambda: shard_problem(hip_sigmoids(ops)))
    mask = p.mask_dev(ops)
    bounds = [p.N * r // W for r in range(W + 1)]
    per_c = [([], []) for _ in SHARD_CS]
    for r in range(W):
        vals, idx = run_sweep(ops, p, SHARD_CS, bounds[r], bounds[r + 1], mask)
        for g in range(len(SHARD_CS)):
            mv, mi, _ = ops.topk_merge(vals[g:g + 1], idx[g:g + 1])
            per_c[g][0].append(mv); per_c[g][1].append(mi)
    for g, c in enumerate(SHARD_CS):
        assert_is_oracle(ops, p, torch.stack(per_c[g][0]), torch.stack(per_c[g][1]), c, (W, c))


# ----------------------------------------------------------------------------- 3. one value overflows, its neighbours do not
def first_round_relists(ops, p, c):
    """stats[0] of macr_score_topk_first_round under the fp32 filter: query blocks whose lists overflowed for this c"""
    stats = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    ops.score_topk(p.kind, dev(p.P), dev(p.user_ids), dev(p.Q), p.K, dev(p.sig_u), dev(p.sig_i), float(c), p.mask_dev(ops),
                   n_splits=1, first_round=True, stats=stats, filter="f32")
    torch.cuda.synchronize()
    return int(stats[0])


def ties_problem(kind):
    rs = np.random.RandomState(4200)
    U, N, d, K = 70, 6000, 64, 20
    P = np.zeros((U, d), np.float32)
    Q = rs.standard_normal((N, d)).astype(np.float32)
    sig_i = ((rs.permutation(N) + 1.0) / (N + 1.0)).astype(np.float32)       # distinct, 1/(N+1) apart, in (0,1)
    sig_i[[5, 4000]] = sig_i.max()                                           # ... but for three equal ones at the top (c < 0)
    sig_i[[5999, 12]] = sig_i.min()                                          # ... and three at the bottom (the top for c > 0)
    mask = random_mask(rs, U, N, 6)
    mask[0] = list(range(0, 40, 2))                                          # query 0 masks every other low id
    return Problem(kind, P, None, Q, K, None, sig_i, mask)


TIE_CS = {0: [0.0, -3.0, 12.5, 40.0], 2: [-3.0, 12.5, 0.0, 40.0], 3: [40.0, -3.0, 12.5, 0.0]}


@pytest.mark.parametrize("slot", sorted(TIE_CS))
@pytest.mark.parametrize("kind", [DIRECT_MINUS, RUBI], ids=["direct_minus", "rubi"])
def test_sweep_one_value_ties_everything_and_overflows(ops, kind, slot, eval_filter):
    """All-zero query rows: the scores are -c sig_i (RUBI: (0 - c) sig_i; DIRECT_MINUS: 0 - c sig_i) for every query.  At
    c = 0 every unmasked item scores 0, equals every threshold and is listed: about 6000 candidates per query against the 1024
    the selection ranks, so that value's overflow flag is set BY CONSTRUCTION and its exact fallback kernel, which no repair
    round precedes here, must rank by ascending id.  At c = -3, 12.5, 40 the scores are as distinct as sig_i (but for the
    deliberate duplicates, ranked by id), the sampled thresholds hold and those lists stay short -- also observed, under the
    fp32 filter, through the sibling entry point macr_score_topk_first_round (a proxy: the sweep itself reports no
    statistics).  The overflowing value sits in slot 0, 2 or 3."""
    cs = TIE_CS[slot]
    p = shared(("ties", kind), lambda: ties_problem(kind))
    vals, idx = run_sweep(ops, p, cs)
    assert_sweep_is_oracle(ops, p, vals, idx, cs, (kind, slot))
    zero = idx[cs.index(0.0)].cpu().numpy()
    assert np.array_equal(zero[0], np.arange(1, 40, 2)[:p.K])                # ascending ids among query 0's unmasked items
    assert np.all(vals[cs.index(0.0)].cpu().numpy() == 0.0)
    if eval_filter == "f32":
        over = {c: first_round_relists(ops, p, c) for c in cs}
        print("ties", kind, "first-round stats[0] per c:", over)
        assert over[0.0] > 0 and all(over[c] == 0 for c in cs if c != 0.0), over


def loose_problem():
    rs = np.random.RandomState(4300)
    U, N, d, K = 300, 3 * 4096, 64, 20
    P = np.abs(rs.standard_normal((U, d)) * 0.5).astype(np.float32)
    Q = np.abs(rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    sig_i = (0.01 + 0.001 * rs.random_sample(N)).astype(np.float32)
    sam = sampled_items(N)
    sig_i[sam] = (0.99 + 0.001 * rs.random_sample(int(sam.sum()))).astype(np.float32)
    return Problem(DIRECT_MINUS, P, None, Q, K, None, sig_i, random_mask(rs, U, N, 10))


LOOSE_CS = {0: [40.0, 0.0, -3.0, -40.0], 1: [0.0, 40.0, -3.0, -40.0], 3: [-40.0, -3.0, 0.0, 40.0]}


@pytest.mark.parametrize("slot", sorted(LOOSE_CS))
def test_sweep_one_value_has_loose_thresholds_and_overflows(ops, slot, eval_filter):
    """All-positive factors, DIRECT_MINUS (y - c sig_i), sig_i ~ 0.99 on the items the sampling pass looks at and ~ 0.01 on the
    rest.  At c = 40 the sampled items score y - 39.6 and everything else y - 0.4: the thresholds learnt from the samples
    admit the other 7/8 of the 12288 items, that value's lists overflow and its fallback kernel ranks.  At c = 0 the branch
    factor drops out; at c = -3 and -40 the sampled items score ABOVE the rest and the thresholds are tight.  That exactly
    c = 40 overflows is asserted under the fp32 filter with macr_score_topk_first_round per value (stats[0] > 0 for 40, == 0
    for the others) -- a proxy through a sibling entry point that shares the sampling pass, the threshold and the list
    capacity with the sweep, which reports no statistics of its own.  The overflowing value sits in slot 0, 1 or 3."""
    cs = LOOSE_CS[slot]
    p = shared("loose", loose_problem)
    vals, idx = run_sweep(ops, p, cs)
    assert_sweep_is_oracle(ops, p, vals, idx, cs, slot)
    if eval_filter == "f32":
        over = {c: first_round_relists(ops, p, c) for c in cs}
        print("loose first-round stats[0] per c:", over)
        assert over[40.0] > 0 and all(over[c] == 0 for c in cs if c != 40.0), over


# ----------------------------------------------------------------------------- the filter margin follows each value's own c
HALF_CELL = 2.0 ** -11           # half a unit in the last place of an fp32 number near 1e4


def margin_problem():
    """Queries e_0, items q0 e_0: the product is q0 itself, exactly, in fp32 and (q0 rounded to 16 significant bits) in the
    two-term bf16 split.  Thirty "top" items sit 2^-22 above a rounding midpoint of (q0 - 1e4), on sampled ids of distinct
    sample classes, so that the thresholds of the sampling pass are their score; every other item scores at least 0.05 less."""
    rs = np.random.RandomState(4600)
    U, N, d, K = 70, 4000, 64, 20
    P = np.zeros((U, d), np.float32); P[:, 0] = 1.0
    Q = np.zeros((N, d), np.float32)
    Q[:, 0] = rs.uniform(-0.5, 0.5, N).astype(np.float32)
    top = 8 * np.arange(30)                                      # window 0 of the sampling pass: item 8 j is sample class j
    assert sampled_items(N)[top].all()
    Q[top, 0] = np.float32(615 * 2.0 ** -10 + HALF_CELL + 2.0 ** -22)        # 0.60107...: exact in fp32, not in 16 bits
    sig_i = np.full(N, 0.5, np.float32)                          # a power of two: the epilogue's product is exact
    return Problem(RUBI, P, None, Q, K, None, sig_i, random_mask(rs, U, N, 6))


MARGIN_CS = [0.0, 1e4, 1e4 + 2.0 ** -10, -1e4]


def test_sweep_filter_margin_is_that_of_each_value(ops, eval_filter):
    """The reduced-precision filters list what scores >= threshold - margin, and the margin holds 1e-6 |c| for the roundings of
    the epilogue: 0.01 at c = 1e4, where one rounding step of (y - c) is 2^-10.  Here the thirty best items have the SAME exact
    score (ranked by id), and the 16-bit product of each lies 2^-22 below its fp32 product, on the other side of a rounding
    midpoint of (y - 1e4): depending on the parity of the cell (hence c = 1e4 and 1e4 + 2^-10) the filter sees them one step,
    2.4e-4, below the threshold.  With the margin of THEIR c they are listed all the same; with the margin of slot 0's c = 0
    (5.6e-5 here) they are lost and the lists come out without them."""
    p = shared("margin", margin_problem)
    top = 8 * np.arange(30)
    for c in MARGIN_CS[1:3]:
        wv, wi, _ = p.want(c)
        free = [[t for t in top if t not in set(p.mask_lists[q])][:p.K] for q in range(p.U)]
        assert all(len(f) == p.K for f in free) and np.array_equal(wi, np.asarray(free))      # the tied top, by ascending id
    vals, idx = run_sweep(ops, p, MARGIN_CS)
    assert_sweep_is_oracle(ops, p, vals, idx, MARGIN_CS, "margin")


# ----------------------------------------------------------------------------- 4. nothing outside [0, n_c) is written
def guard_problem(N, sigmoid):
    rs = np.random.RandomState(4400 + N)
    U, d, K = 300, 64, 20
    P = (rs.standard_normal((U + 11, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.5).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    user_ids = rs.permutation(U + 11)[:U].astype(np.int32)
    return Problem(RUBI_BOTH, P, user_ids, Q, K, sigmoid(P, wu, user_ids), sigmoid(Q, w), random_mask(rs, U, N, 12, heavy=(3,)))


GUARD_CS = [40.0, -3.0, 12.5]


@pytest.mark.parametrize("N", [900, 2500], ids=["lists-everything", "samples"])
@pytest.mark.parametrize("n_c", [1, 2, 3])
def test_sweep_writes_nothing_past_its_n_c_slices(ops, n_c, N, eval_filter):
    """macr_score_topk_sweep called through the C ABI with n_c < MACR_MAX_SWEEP: the outputs are 4 U K long and the workspace
    is exactly macr_score_topk_sweep_workspace_bytes(n_c) followed, in the same allocation, by a guard as long as the
    workspaces of the absent values; the output tails and the guard keep their sentinel bytes (the kernels' slots g >= n_c
    alias slot 0 and must stay unused), and the first n_c slices are the oracle's."""
    from macr_amd import _lib
    L = _lib.lib()
    p = shared(("guard", N), lambda: guard_problem(N, hip_sigmoids(ops)))
    cs = GUARD_CS[:n_c]
    U, K, d = p.U, p.K, p.d
    one = L.macr_score_topk_sweep_workspace_bytes(U, N, d, 1)
    need = L.macr_score_topk_sweep_workspace_bytes(U, N, d, n_c)
    assert need == n_c * one and one % 256 == 0
    guard = (_lib.MAX_SWEEP - n_c) * one + 4096
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    out_val = torch.full((_lib.MAX_SWEEP, U, K), 12345.0, dtype=torch.float32, device="cuda")
    out_idx = torch.full((_lib.MAX_SWEEP, U, K), -77, dtype=torch.int32, device="cuda")
    Pd, uid, Qd, su, si, cd = dev(p.P), dev(p.user_ids), dev(p.Q), dev(p.sig_u), dev(p.sig_i), dev(np.asarray(cs, np.float32))
    mask = p.mask_dev(ops)
    bits = mask.mask_bits(U, N, 0)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.macr_score_topk_sweep(p.kind, ops.eval_filter_code(eval_filter), U, N, d, ptr(Pd), ptr(uid), ptr(Qd), ptr(su), ptr(si),
                                 n_c, ptr(cd), ptr(mask.ptr), ptr(mask.idx), ptr(bits), 0, K, ptr(out_val), ptr(out_idx),
                                 ptr(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK, L.macr_last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the guard behind the workspace was written"
    assert bool((out_val[n_c:] == 12345.0).all()) and bool((out_idx[n_c:] == -77).all()), "an output slice >= n_c was written"
    assert_sweep_is_oracle(ops, p, out_val[:n_c], out_idx[:n_c], cs, (n_c, N))


# ----------------------------------------------------------------------------- 5. replay follows c
class SweepTap(object):
    """Gets at the LISTS of an Evaluator's sweep (its methods return metrics only).  Every ops.score_topk_sweep call of the
    evaluator is recorded by its group size; the call made while a graph is captured leaves the graph's own output tensors
    here, which hold the replayed rankings after each replay.  After every replay the group's values of c (read back from the
    device array the kernels read) and its lists are copied into `seen`.

    A context manager that owns the evaluator: on the way out, passed or failed, the captured graphs and the tensors of their
    memory pools are released there and then.  The evaluator must not end up in a reference cycle (the tap hangs on the
    CLASS's _replay, not on the instance) or in a kept traceback: a graph that the garbage collector destroys later may be
    destroyed in the middle of another test's stream capture."""

    def __init__(self, ev, ops, monkeypatch):
        self.ev, self.seen, self._last = ev, [], {}
        real_sweep, real_replay = ops.score_topk_sweep, type(ev)._replay

        def sweep(kind, users_tab, user_ids, items, K, sig_u, sig_i, c_dev, *a, **kw):
            vals, idx = real_sweep(kind, users_tab, user_ids, items, K, sig_u, sig_i, c_dev, *a, **kw)
            self._last[c_dev.numel()] = (c_dev, vals, idx)
            return vals, idx

        def replay(entry):
            out = real_replay(entry)
            n = next(k[1] for k, e in self.ev._graphs.items() if e is entry)     # key: ("sweep", group size, ...)
            c_dev, vals, idx = self._last[n]
            torch.cuda.synchronize()
            self.seen.append((c_dev.cpu().numpy().tolist(), vals.clone(), idx.clone()))
            return out
        monkeypatch.setattr(ops, "score_topk_sweep", sweep)
        monkeypatch.setattr(type(ev), "_replay", staticmethod(replay))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self._last.clear()
        self.seen = [(cs, v.cpu(), i.cpu()) for cs, v, i in self.seen]
        self.ev._graphs.clear()                  # the CUDAGraph objects die here, by reference count, outside any capture
        self.ev = None
        return False


def replay_problem(sigmoid):
    rs = np.random.RandomState(4500)
    U, N, d, K = 300, 2500, 64, 20
    P = (rs.standard_normal((U + 40, d)) * 0.4).astype(np.float32)
    Q = (rs.standard_normal((N, d)) * 0.4).astype(np.float32)
    B = (Q + rs.standard_normal((N, d)) * 0.3).astype(np.float32)            # the "ego" item rows of the one-branch call
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    user_ids = np.sort(rs.choice(U + 40, U, replace=False)).astype(np.int32)
    mask = random_mask(rs, U, N, 25, heavy=(9,))
    p = Problem(RUBI_BOTH, P, user_ids, Q, K, sigmoid(P, wu, user_ids), sigmoid(Q, w), mask)
    p.branch = Problem(RUBI, P, user_ids, Q, K, None, sigmoid(B, w), mask)   # scores from Q, branch factors from B
    p.B, p.w, p.wu = B, w, wu
    p.gt = [sorted(rs.choice(N, 5, replace=False).tolist()) for _ in range(U)]
    return p


C_POOL = [-5.0, -3.0, -1.5, 0.0, 0.5, 2.0, 5.0, 7.5, 12.5, 20.0, 30.0, 40.0]


def groups_of(cs):
    return [[float(np.float32(c)) for c in cs[a:a + 4]] for a in range(0, len(cs), 4)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
def test_replayed_sweep_ranks_the_new_values(ops, n, eval_filter, monkeypatch):
    """Evaluator.test_mf_sweep with graphs on, twice with different values of the same count (groups of four, then the rest:
    one captured graph per group size, the values in a device array): every replay -- the second call's included, which
    launches nothing but replays -- leaves the oracle's LISTS for the values it was given, not only their metrics."""
    from macr_amd.evaluator import Evaluator
    p = shared("replay", lambda: replay_problem(hip_sigmoids(ops)))
    ev = Evaluator(p.mask_lists, p.gt, p.N, torch.device("cuda"))
    assert ev.use_graph and ev.filter == eval_filter
    Pd, uid, Qd, w, wu = dev(p.P), dev(p.user_ids), dev(p.Q), dev(p.w), dev(p.wu)
    first, second = C_POOL[:n], C_POOL[::-1][:n]
    assert all(a != b for a, b in zip(first, second))
    with SweepTap(ev, ops, monkeypatch) as tap:
        for cs in (first, second):
            res = ev.test_mf_sweep(p.kind, Pd, uid, Qd, [5, p.K], w, wu, cs)
            assert len(res) == n
        n_graphs = len([k for k in ev._graphs if k[0] == "sweep"])
    assert [s[0] for s in tap.seen] == groups_of(first) + groups_of(second)  # every group came out of a replay, in order
    assert n_graphs == len(set(len(g) for g in groups_of(first)))            # one graph per group size, captured once
    for cs, vals, idx in tap.seen:
        assert_sweep_is_oracle(ops, p, vals.cuda(), idx.cuda(), cs, (n, cs))


def test_replayed_one_branch_sweep_reads_the_branch_table(ops, eval_filter, monkeypatch):
    """The LightGCN flavour with a separate branch table (rubi_ratings2: SCORE_RUBI, branch factors from the ego item rows,
    scores from the propagated ones), twice: the lists are the oracle's with sig_i taken from the BRANCH table."""
    from macr_amd.evaluator import Evaluator
    full = shared("replay", lambda: replay_problem(hip_sigmoids(ops)))
    p = full.branch
    ev = Evaluator(p.mask_lists, full.gt, p.N, torch.device("cuda"))
    Pd, uid, Qd, Bd, w, wu = dev(p.P), dev(p.user_ids), dev(p.Q), dev(full.B), dev(full.w), dev(full.wu)
    assert not np.array_equal(p.sig_i, full.sig_i)
    with SweepTap(ev, ops, monkeypatch) as tap:
        for cs in ([0.0, 20.0, 40.0], [30.0, -3.0, 12.5]):
            res = ev.test_lgcn_sweep(p.kind, Pd, uid, Qd, [5, p.K], w, wu, cs, branch=Bd)
            assert len(res) == 3
    assert [s[0] for s in tap.seen] == [[0.0, 20.0, 40.0], [30.0, -3.0, 12.5]]
    for cs, vals, idx in tap.seen:
        assert_sweep_is_oracle(ops, p, vals.cuda(), idx.cuda(), cs, cs)
