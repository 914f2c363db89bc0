"""The deferred MF step against the complete one, BIT FOR BIT, under MACR_STEP_DETERMINISTIC (-m gpu).

A deferred step (MACR_STEP_DEFER) leaves its dense Adam pass pending.  The next step's forward looks one update ahead in
registers (k_pair_fwd<LPR, 1>), the pass itself rides as extra blocks of that step's (B,B) launch (k_bxb<R, FULL, 1>,
adam_block<true>), and flush() runs it stand-alone (k_adam_dense).  train_kernels.hip promises that the three give the same bits;
the deterministic mode takes every order-of-arrival effect out of the gradients, so the promise can be checked exactly.  The
problems are those of tests/mf_det_cases.py; every state is MFState(deterministic=True), every kind a (B,B) kind.

1. the riding pass stores what the stand-alone pass stores: tables, branch vectors and every slot, for the pass of step 0
   (riding in step 1) and the pass of step 1 (riding in step 2: all eight partial rows of the branch vectors in use).
2. the look-ahead sees the rows the pass stores: the seven arrays pair_fwd leaves in the workspace (macr_test_pair_ws_layout; no
   kernel of an MF step writes `fwd` after pair_fwd: k_bxb and the backward kernels take it as const, only LightGCN's ego
   branch stages scalars over it) and the step's three losses, from stored rows (k_pair_fwd<LPR, 0> after a flush) and from
   looked-ahead rows (k_pair_fwd<LPR, 1>).
3. six deferred steps ended by a flush leave the losses of every step, the tables, the slots and the beta powers of six complete
   steps; so do deferred sequences that the host cuts short (an explicit flush, a change of kind, a change of B).

Before the look-ahead summed the branch vectors' partial rows in the pass's association (d = 256: the pass adds
(((g0+g4)+(g1+g5))+(g2+g6))+(g3+g7), the look-ahead added the eight rows in turn), 1 held everywhere -- both passes are
adam_block -- and 2 and 3 failed at B257 and nowhere else: 2 for rubibceboth (7 columns of `a`, at most 2 ulp), 3 for rubibceboth
(P of the six steps: 83 elements, at most 64 ulp) and, across the change of B, for rubi as well.  The sigmoids of the branch
logits absorb most of a last-bit difference in w, which is why rubibce showed nothing at these sizes.
"""
import functools

import pytest
import torch

from mf_det_cases import BXB_KINDS, SHAPES, STATE_NAMES, STEPS, bits_equal, dev, device_batches, fresh, problem, run, snapshot

pytestmark = pytest.mark.gpu

PASS_SHAPES = [s for s in SHAPES if s != "B8448"]
# what a pass stores (the gradient scratch, the row flags and the beta powers belong to the step that is still pending)
PASS_STORES = ("_P", "_Q", "mP", "vP", "mQ", "vQ", "w", "wu", "mw", "vw", "mwu", "vwu")
SEQ_SHAPES = ("B300", "B257")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def deferred(ops, shape, kind_name, n):
    """a fresh state after deferred steps 0 .. n-1: the pass of step n-1 pending"""
    state = fresh(ops, shape, True)
    for u, i, j in device_batches(shape)[:n]:
        state.step(getattr(ops, kind_name), u, i, j, defer=True)
    assert state.pending_B == SHAPES[shape][0] and state._seq_lazy is None
    return state


def ulps(a, b):
    """largest distance of two float32 tensors in units in the last place (finite values)"""
    key = lambda x: torch.where(x.view(torch.int32) < 0, -(x.view(torch.int32) & 0x7FFFFFFF), x.view(torch.int32)).to(torch.int64)
    return int((key(a) - key(b)).abs().max())


def assert_pass_stores_equal(a, b, where):
    for n in PASS_STORES:
        x, y = getattr(a, n), getattr(b, n)
        assert bits_equal(x, y), (where, n, "%d elements differ, at most %d ulp" % (int((x != y).sum()), ulps(x, y)))


# ----------------------------------------------------------------------------- 1. the riding pass is the stand-alone pass
@pytest.mark.parametrize("kind_name", BXB_KINDS)
@pytest.mark.parametrize("shape", PASS_SHAPES)
def test_riding_pass_stores_what_the_stand_alone_pass_stores(ops, shape, kind_name):
    kind = getattr(ops, kind_name)
    batches = device_batches(shape)
    initial = problem(shape)
    for n in (1, 2):                                    # the pass of step n - 1: alone in A, riding in step n in B
        a, b = deferred(ops, shape, kind_name, n), deferred(ops, shape, kind_name, n)
        assert_pass_stores_equal(a, b, (shape, kind_name, n, "before the pass"))
        ops.timing_begin()
        a.flush()
        alone = {k for k, _ in ops.timing_end(64)}
        ops.timing_begin()
        b.step(kind, *batches[n], defer=True)
        riding = {k for k, _ in ops.timing_end(64)}
        assert "adam_dense" in alone and "bxb+adam" in riding and "adam_dense" not in riding, (alone, riding)
        assert b.pending_B and not a.pending_B
        assert_pass_stores_equal(a, b, (shape, kind_name, n))
        # (the pass ran: every row of the batches so far moved, and so did the branch vector every kind trains)
        for tab, col, first in ((b._P, 0, initial[0]), (b._Q, 1, initial[1])):
            rows = torch.unique(torch.cat([x[col] for x in batches[:n]]).long())
            assert bool((tab[rows] != dev(first)[rows]).any(dim=1).all()), "rows of the batch the riding pass left alone"
        assert bool((b.w != dev(initial[2])).any())


# ----------------------------------------------------------------------------- 2. the look-ahead sees the rows the pass stores
def fwd_of(ops, state, B):
    """the (7, B) outputs of the last pair_fwd, as they lie in the state's workspace"""
    off, Bp = ops.test_pair_ws_layout(B, state.d, state.deterministic)
    assert Bp >= B and Bp % 256 == 0 and off % 4 == 0 and off + 7 * Bp * 4 <= state.ws.numel(), (off, Bp)
    return state.ws[off:off + 7 * Bp * 4].view(torch.float32).view(7, Bp)[:, :B].clone()


@pytest.mark.parametrize("kind_name", BXB_KINDS)
@pytest.mark.parametrize("shape", PASS_SHAPES)
def test_look_ahead_forward_equals_the_forward_on_stored_rows(ops, shape, kind_name):
    kind = getattr(ops, kind_name)
    B, d = SHAPES[shape][:2]
    for n in (1, 2):                                    # step n on the rows of step n - 1's pass: stored by A, looked ahead by B
        u, i, j = device_batches(shape)[n]
        a, b = deferred(ops, shape, kind_name, n), deferred(ops, shape, kind_name, n)
        a.flush()
        ops.timing_begin()
        la = a.step(kind, u, i, j, defer=True).clone()          # k_pair_fwd<LPR, 0> on the rows k_adam_dense stored
        assert "bxb" in {k for k, _ in ops.timing_end(64)}
        ops.timing_begin()
        lb = b.step(kind, u, i, j, defer=True).clone()          # k_pair_fwd<LPR, 1> on rows updated in registers
        assert "bxb+adam" in {k for k, _ in ops.timing_end(64)}
        fa, fb = fwd_of(ops, a, B), fwd_of(ops, b, B)
        # the region is pair_fwd's: p and n are the dots of the rows A holds (its own pass is still pending, so they are the rows
        # its forward read); an fp32 dot of d products in any order is within d * 2^-24 * sum |products| of the exact one
        eu, ei, ej = (t.double() for t in (a._P[u.long()], a._Q[i.long()], a._Q[j.long()]))
        for k, other in ((0, ei), (1, ej)):
            err = (fa[k].double() - (eu * other).sum(1)).abs()
            assert bool((err <= d * 2.0 ** -24 * (eu * other).abs().sum(1)).all()), (shape, kind_name, n, "fwd[%d] is not the pair dots" % k)
        names = ("p", "n", "a", "b", "sig_si", "sig_sj", "sig_su / 1 - sig(si - sj), signed")
        for k in range(7):
            assert bits_equal(fa[k], fb[k]), (shape, kind_name, n, names[k], "%d columns differ, at most %d ulp" % (
                int((fa[k].view(torch.int32) != fb[k].view(torch.int32)).sum()), ulps(fa[k], fb[k])))
        assert bits_equal(la, lb), (shape, kind_name, n, la, lb)


# ----------------------------------------------------------------------------- 3. the two forms give the same trajectory
@functools.lru_cache(maxsize=None)
def complete(ops, shape, kind_name):
    """six complete steps, once per problem and kind -> (losses (6, 3), final state); read only"""
    return run(ops, shape, kind_name, True, defer=False)


def assert_same_trajectory(got, want, where):
    (lg, sg), (lw, sw) = got, want
    assert bool(torch.isfinite(lw).all()), lw
    for t in range(lw.shape[0]):
        assert bits_equal(lg[t], lw[t]), (where, "losses of step %d" % t, lg[t], lw[t])
    for n in STATE_NAMES:
        assert bits_equal(sg[n], sw[n]), (where, n, "%d elements differ, at most %d ulp" % (int((sg[n] != sw[n]).sum()), ulps(sg[n], sw[n])))


@pytest.mark.parametrize("kind_name", BXB_KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_deferred_sequence_equals_complete_steps(ops, shape, kind_name):
    assert_same_trajectory(run(ops, shape, kind_name, True, defer=True), complete(ops, shape, kind_name), (shape, kind_name))


def sequence(ops, shape, plan, defer):
    """one step per entry of plan = (kind name, triples of the batch used, flush after the step) -> (losses, final state)"""
    state = fresh(ops, shape, True)
    losses = []
    for (kind_name, n, flush), (u, i, j) in zip(plan, device_batches(shape)):
        losses.append(state.step(getattr(ops, kind_name), u[:n], i[:n], j[:n], defer=defer).clone())
        assert state.pending_B == (n if defer else 0)
        if flush:
            state.flush()
    state.flush()
    return torch.stack(losses), snapshot(state)


@pytest.mark.parametrize("kind_name", BXB_KINDS)
@pytest.mark.parametrize("shape", SEQ_SHAPES)
def test_deferred_sequence_with_a_flush_in_the_middle(ops, shape, kind_name):
    B = SHAPES[shape][0]
    plan = [(kind_name, B, t == 2) for t in range(STEPS)]
    assert_same_trajectory(sequence(ops, shape, plan, True), complete(ops, shape, kind_name), (shape, kind_name))


@pytest.mark.parametrize("shape", SEQ_SHAPES)
def test_deferred_sequence_across_a_change_of_kind(ops, shape):
    """MFState.step flushes the pending rubibce pass before the first rubibceboth step, where w_user's segment appears"""
    B = SHAPES[shape][0]
    plan = [("LOSS_RUBIBCE" if t < 3 else "LOSS_RUBIBCEBOTH", B, False) for t in range(STEPS)]
    got, want = sequence(ops, shape, plan, True), sequence(ops, shape, plan, False)
    assert bool((want[1]["mwu"] != 0).any()) and bool((want[1]["mw"] != 0).any())          # (both branch vectors trained)
    assert_same_trajectory(got, want, (shape, "rubibce -> rubibceboth"))


@pytest.mark.parametrize("kind_name", BXB_KINDS)
@pytest.mark.parametrize("shape", SEQ_SHAPES)
def test_deferred_sequence_across_a_change_of_batch_size(ops, shape, kind_name):
    """step 3 on the first B - 7 triples of its batch: the host flushes the pending pass of B triples before it, and again
    before step 4 returns to B"""
    B = SHAPES[shape][0]
    plan = [(kind_name, B - 7 if t == 3 else B, False) for t in range(STEPS)]
    assert_same_trajectory(sequence(ops, shape, plan, True), sequence(ops, shape, plan, False), (shape, kind_name, "B - 7"))
