"""The problems of the bit-reproducible MF step (MFState(deterministic=True)), shared by tests/test_gpu_deterministic.py (each form
against itself and against the CPU restatements) and tests/test_gpu_deferred_forms.py (the deferred form against the complete one).

Every shape is the smallest that reaches a place where the order of a sum could leak, or where the Adam pass riding in the (B,B)
launch could differ from the stand-alone one; the hot rows are built by hand, so their reference counts are known (chunks of
k_seg_reduce: 16 references, 8 at d = 32):

    B300   d64   40 x 50      i[:150] = 0, j[150:225] = 1, u[:150] = 3: more batch positions than users (drawn with
                              replacement); runs of 150 and more -- ten chunks -- in BOTH tables.  By default the small-batch
                              atomic path.  Both tables smaller than one block of the Adam pass
    B96    d32   200 x 100    item 0 48 times: chunks of 8
    B257   d256  300 x 80     item 0 130 times; one lane group per wave; the pass sums the branch vectors' eight partial rows in
                              four lane groups of two
    B4096  d64   5003 x 1201  item 0 2048 times as positive, item 1 1024 times as negative: full 256-blocks (the default step
                              runs neutral blocks for the BCE kinds), 256 backward blocks = 32 per branch-vector slot
    B8448  d128  9001 x 1201  item 0 1000 times: by default the staged, indexed route with 16 work items on one row
    B100   d128  70001 x 37   item 0 40 times.  The user table is 2187.5 blocks of the Adam pass (1024 float4 each) behind a
                              (B,B) launch of 4 blocks, the last one partial; the item table one full block and one partial; B
                              is no multiple of 256
"""
import functools

import numpy as np
import torch

LR, DECAY, ALPHA, BETA, BS = 1e-3, 1e-5, 1e-2, 1e-3, 1024
STEPS = 6
STATE_NAMES = ("P", "Q", "w", "wu", "mP", "vP", "mQ", "vQ", "mw", "vw", "mwu", "vwu", "adam_pow")
KINDS = ("LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH", "LOSS_RUBIBCE", "LOSS_BPR", "LOSS_RUBIBPR")
BXB_KINDS = ("LOSS_RUBIBCEBOTH", "LOSS_RUBIBCE", "LOSS_RUBIBPR")

# name -> (B, d, n_users, n_items, [(array, start, stop, row)] hot runs written over the random batch)
SHAPES = {
    "B300": (300, 64, 40, 50, (("i", 0, 150, 0), ("j", 150, 225, 1), ("u", 0, 150, 3))),
    "B96": (96, 32, 200, 100, (("i", 0, 48, 0),)),
    "B257": (257, 256, 300, 80, (("i", 0, 130, 0),)),
    "B4096": (4096, 64, 5003, 1201, (("i", 0, 2048, 0), ("j", 2048, 3072, 1))),
    "B8448": (8448, 128, 9001, 1201, (("i", 0, 1000, 0),)),
    "B100": (100, 128, 70001, 37, (("i", 0, 40, 0),)),
}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a writable copy: the problems' arrays are read-only)


@functools.lru_cache(maxsize=None)
def problem(shape):
    """tables, branch vectors and STEPS batches (a fresh draw per step, the shape's hot runs in every one)"""
    B, d, n_users, n_items, hot = SHAPES[shape]
    rs = np.random.RandomState(B + d)
    P = (rs.standard_normal((n_users, d)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    w, wu = (rs.standard_normal(d) * 0.3).astype(np.float32), (rs.standard_normal(d) * 0.3).astype(np.float32)
    batches = []
    for _ in range(STEPS):
        b = dict(u=rs.choice(n_users, B, replace=B > n_users).astype(np.int32), i=rs.randint(0, n_items, B).astype(np.int32),
                 j=rs.randint(0, n_items, B).astype(np.int32))
        for name, lo, hi, row in hot:
            b[name][lo:hi] = row
        o = rs.permutation(B)                                       # the hot references spread over the batch's blocks
        batches.append(tuple(b[k][o] for k in ("u", "i", "j")))
    for a in (P, Q, w, wu) + tuple(x for b in batches for x in b):
        a.setflags(write=False)
    return P, Q, w, wu, tuple(batches)


@functools.lru_cache(maxsize=None)
def device_batches(shape):
    return tuple(tuple(dev(x) for x in b) for b in problem(shape)[4])


def hyper(ops):
    return ops.make_hyper(LR, DECAY, ALPHA, BETA, BS)


def fresh(ops, shape, deterministic):
    P, Q, w, wu, _ = problem(shape)
    return ops.MFState(dev(P), dev(Q), dev(w), dev(wu), hyper(ops), SHAPES[shape][0], deterministic=deterministic)


def snapshot(state):
    return {n: getattr(state, n).clone() for n in STATE_NAMES}


def assert_clean(state, where):
    assert float(state.gP.abs().max()) == 0.0 and float(state.gQ.abs().max()) == 0.0, "%s: gradient scratch not zero" % (where,)
    assert int(state.tP.abs().sum()) == 0 and int(state.tQ.abs().sum()) == 0, "%s: row flags set" % (where,)


def run(ops, shape, kind_name, deterministic, defer=False, first=None):
    """STEPS steps from the problem's initial arrays -> (losses of every step (STEPS, 3), final state); first: dict that
    receives mP, mQ, mw, mwu after the first step (complete steps only)"""
    kind = getattr(ops, kind_name)
    state = fresh(ops, shape, deterministic)
    assert state.deterministic == deterministic and (state.lazy_period == 1 or not deterministic)
    losses = []
    for t, (u, i, j) in enumerate(device_batches(shape)):
        losses.append(state.step(kind, u, i, j, defer=defer).clone())
        if defer:
            assert state.pending_B == SHAPES[shape][0] and state._seq_lazy is None
        elif deterministic:
            assert_clean(state, (shape, kind_name, t))
        if first is not None and t == 0:
            first.update({n: getattr(state, n).clone() for n in ("mP", "mQ", "mw", "mwu")})
    state.flush()
    if deterministic:
        assert_clean(state, (shape, kind_name, "end"))
    return torch.stack(losses), snapshot(state)


def bits_equal(a, b):
    """same shape, same bits (NaNs of equal payload included)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
