"""The lazy dense Adam pass (include/macr_hip.h: macr_lazy_adam) over 330 steps: past the wrap of the 256-slot lr_t ring, with
rows a whole period (64 steps, + the pending step in deferred mode) behind when they are read, on tables of fewer chunks than
the period -- against the per-step dense pass of the same library bit for bit, against the schedule model of tests/lazy_ref.py
stamp for stamp, and (rows no batch references) against the fp64 closed form of the recurrence.
tests/test_lazy_ref_cpu.py shows on the same inputs that the full lag and the wrap are really reached:

                         max lag   readers at full lag across ring slots 255 -> 0, at steps
  sharded   d = 32       64        gather 257-264, 267, ... 317 (28 steps); sweep 256-318
  sharded   d = 256      64        gather 257-261; sweep 257-262, 284
  deferred  d = 32       65        forward look-ahead and riding pass 257-262
  deferred  d = 256      65        forward look-ahead and riding pass 257-281
  (period 7: max lag 7 / 8; nobody ever walks more than K ring slots; at most 42 references of a row in a sharded batch)"""
import numpy as np
import pytest
import torch

import lazy_ref as lr
from test_gpu_lazy_adam import _MF_NAMES, _batch, _lockstep, _mf_states, _models, _same_state

pytestmark = pytest.mark.gpu

IDLE = lr.IDLE


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stamp_history(form, sizes, d, batches, flush_at=None):
    """lazy_ref's stamps after every step, per table an int32 (steps + 1, n) device tensor"""
    out = []
    for k, K in enumerate(lr.PERIODS[1:]):
        hist, _, _ = lr.run_schedule(form, sizes, d, K, batches, lr.FLUSH_AT if k == 2 and flush_at else None,
                                     lr.READ_ALL_AT if form == "sharded" else ())
        out.append([_dev(h.astype(np.int32)) for h in hist])
    return out


def _plant_idle_slots(tables, d):
    """non-zero Adam slots under the last IDLE rows of both tables of every model, before the first step.
    tables: per model ((P, mP, vP), (Q, mQ, vQ)).  Returns per table (theta_0, m_0, v_0) of those rows."""
    start = []
    for tab in range(2):
        m0, v0 = lr.idle_slots(11 + tab, d)
        for t in tables:
            t[tab][1][-IDLE:] = _dev(m0)
            t[tab][2][-IDLE:] = _dev(v0)
        start.append((tables[0][tab][0][-IDLE:].cpu().numpy().copy(), m0, v0))
    return start


def _check_idle_rows(tables, start, T, record_property):
    """theta, m, v of the idle rows of every model after T steps against the closed form; bound: 4 x what the same steps in
    float32 on the CPU deviate from it + one float32 ulp (the device's sqrt / rcp + Newton path is within 1 ulp of IEEE).
    Measured on an MI355X, T = 330, max |. - fp64| over the 12 rows (user table / item table); the GPU's figure, the largest
    over the dense and every lazy model, came out EQUAL to the CPU float32 run's in every case:
                          theta                  m                      v
      sharded   d = 32    4.76e-7 / 4.44e-7      1.86e-23 / 2.28e-23    1.16e-10 / 8.74e-11
      sharded   d = 256   6.31e-7 / 5.34e-7      2.58e-23 / 2.44e-23    1.02e-10 / 1.08e-10
      deferred  d = 32    5.87e-7 / 4.67e-7      (m_0, v_0 and so m, v as in the sharded runs)
      deferred  d = 256   9.32e-7 / 7.48e-7
    against rows that move by 1e-3 and more."""
    for tab, (theta0, m0, v0) in enumerate(start):
        want, bounds, dev = lr.idle_bounds(theta0, m0, v0, T)
        worst = [0.0, 0.0, 0.0]
        for k, t in enumerate(tables):
            got = [x[-IDLE:].cpu().numpy() for x in t[tab]]
            assert np.array_equal(got[0][[3, 8]], theta0[[3, 8]]), ("model %d table %d: a row with m = v = 0 moved" % (k, tab))
            for q in range(3):
                err = np.abs(got[q].astype(np.float64) - want[q])
                worst[q] = max(worst[q], float(err.max()))
                print("idle rows: model %d table %d %s: |gpu - fp64| = %.3e, |fp32 cpu - fp64| = %.3e" % (k, tab, "theta m v".split()[q], err.max(), dev[q]))
                assert (err <= bounds[q]).all(), (k, tab, "theta m v".split()[q], float(err.max()), dev[q])
        for q, name in enumerate(("theta", "m", "v")):
            record_property("idle_table%d_%s_cpu_fp32_dev" % (tab, name), dev[q])
            record_property("idle_table%d_%s_gpu_dev" % (tab, name), worst[q])
        assert np.abs(want[0] - theta0).max() > 1e-3           # (the rows moved by thousands of those deviations)


# ---------------------------------------------------------------------------------------------------------------------
# sharded form: k_rows_gather_owned<LAZY>, k_adam_lazy, k_lazy_rows, the flush
# ---------------------------------------------------------------------------------------------------------------------
def _rows_as_of_now_write_nothing(m, dense, step):
    state = (m._P, m._mP, m._vP, m.stP, m._Q, m._mQ, m._vQ, m.stQ)
    before = [t.clone() for t in state]
    for tab, want in (("P", dense._P), ("Q", dense._Q)):
        every = torch.arange(want.shape[0], dtype=torch.int32, device="cuda")
        got = m.backend.lazy_rows(m, tab, every)
        if not torch.equal(got, want):
            bad = (got != want).any(1).nonzero().flatten()
            st = (m.stP if tab == "P" else m.stQ)[bad]
            raise AssertionError("step %d, K = %d, table %s: %d rows differ, first row %d (stamp %d), max |diff| %g" % (
                step, m.lazy_period, tab, bad.numel(), int(bad[0]), int(st[0]), float((got - want).abs().max())))
    for a, b in zip(before, state):
        assert torch.equal(a, b), "lazy_rows wrote something"


@pytest.mark.parametrize("d", [32, 256])
def test_sharded_lazy_pass_over_the_ring_wrap_at_full_lag(d, record_property):
    """RowShardedMF, world 1, periods 1 / 7 / 64 / 64 on the same gradients (_lockstep: the gather equality every step).  User
    table: 3 chunks, the last one partial (fewer than 7: most sweep phases lie beyond the last chunk); item table: 70 chunks +
    a partial one.  lazy_rows over every row (steps 250-262 and every 16th) equals the dense tables and writes nothing; stamps
    equal lazy_ref's after every step; the fourth model is flushed after step 258 (stamps from 195 on, across the wrap).
    The last 12 rows of each table are in no batch: _check_idle_rows."""
    from macr_amd import ops
    n_users, n_items = lr.SHARDED_SHAPES[d]
    models, _ = _models(n_users, n_items, d, lr.PERIODS, ops.LOSS_RUBIBCEBOTH)
    dense, lazies = models[0], models[1:]
    tables = [((m._P, m._mP, m._vP), (m._Q, m._mQ, m._vQ)) for m in models]
    start = _plant_idle_slots(tables, d)
    batches, raw = lr.sharded_batches(d), lr.sharded_batches(d, raw=True)
    hists = _stamp_history("sharded", (n_users, n_items), d, batches, flush_at=True)
    rs = np.random.RandomState(lr.BATCH_SEED)
    for n in range(1, lr.STEPS + 1):
        drawn = _batch(rs, n_users - IDLE - lr.SHARDED_COLD[0], n_items - IDLE - lr.SHARDED_COLD[1], lr.SHARDED_B)
        assert all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(drawn, raw[n - 1]))      # lazy_ref's batches are _batch's
        _lockstep(dense, lazies, *[_dev(a) for a in batches[n - 1]])
        if n in lr.READ_ALL_AT:
            for m in lazies:
                _rows_as_of_now_write_nothing(m, dense, n)
        if n == lr.FLUSH_AT:
            assert lazies[2]._stale and int(lazies[2].stQ.min()) == n - 63 < 255      # (the flush walks across the wrap)
            _same_state(lazies[2], dense)
        for m, h in zip(lazies, hists):
            for tab, st in enumerate((m.stP, m.stQ)):
                if not torch.equal(st, h[tab][n]):
                    bad = (st != h[tab][n]).nonzero().flatten()
                    raise AssertionError("step %d, K = %d, table %d: %d stamps differ, first row %d: %d, lazy_ref %d" % (
                        n, m.lazy_period, tab, bad.numel(), int(bad[0]), int(st[bad[0]]), int(h[tab][n][bad[0]])))
    for m in lazies:
        _same_state(m, dense)
        assert int(m.stP.min()) == lr.STEPS == int(m.stP.max()) and int(m.stQ.min()) == lr.STEPS == int(m.stQ.max())
    _check_idle_rows(tables, start, lr.STEPS, record_property)


# ---------------------------------------------------------------------------------------------------------------------
# deferred MF form: k_pair_fwd<2>, adam_lazy_scan_block, macr_mf_train_flush_lazy
# ---------------------------------------------------------------------------------------------------------------------
def _mf_tables(states):
    return [((s._P, s.mP, s.vP), (s._Q, s.mQ, s.vQ)) for s in states]


def _mf_same(s, dense, where):
    for name in _MF_NAMES:
        x, y = getattr(s, name), getattr(dense, name)
        assert torch.equal(x, y), (where, name, float((x - y).abs().max()))
    assert int(s.tP.abs().sum()) == 0 and int(s.tQ.abs().sum()) == 0
    assert float(s.gP.abs().max()) == 0.0 and float(s.gQ.abs().max()) == 0.0


def _mf_stamps_are(s, want, where):
    _, sp, sq = s._lazy_bufs
    for tab, (st, w) in enumerate(zip((sp, sq), want)):
        if not torch.equal(st, w):
            bad = (st != w).nonzero().flatten()
            raise AssertionError("%s, K = %d, table %d: %d stamps differ, first row %d: %d, lazy_ref %d" % (
                where, s.lazy_period, tab, bad.numel(), int(bad[0]), int(st[bad[0]]), int(w[bad[0]])))


@pytest.mark.parametrize("d", [32, 256])
def test_mf_lazy_sequence_over_the_ring_wrap_at_full_lag(d, record_property):
    """MFState, defer=True, periods 1 / 7 / 64 / 64, B = 128 without a repeated row (every atomic lands on a zero): the losses
    of every step equal the dense sequence's -- the forward looks from each row's stamp to the pending step, for lazy_ref's cold
    rows 64 idle steps + the pending one, in calls 257 ... across the wrap -- and the stamps equal lazy_ref's (one step behind
    the counter).  The fourth model is flushed after call 258 and carries on as a new sequence; its dense partner is a second
    dense model flushed at the same call, so that both sides of every comparison took the same calls.
    d = 32: 300 users, 700 items: 3 and 6 chunks for periods 7 and 64.  The last 12 rows of each table are in no batch:
    _check_idle_rows, on all five models."""
    from macr_amd import ops
    kind_name, n_users, n_items = lr.DEFERRED_SHAPES[d]
    kind, B = getattr(ops, kind_name), lr.DEFERRED_B
    states, _ = _mf_states(n_users, n_items, d, B, [1, 1] + lr.PERIODS[1:])
    partner = {2: 0, 3: 0, 4: 1}                                # lazy model -> the dense model it is compared with
    start = _plant_idle_slots(_mf_tables(states), d)
    batches = lr.deferred_batches(d)
    hists = _stamp_history("deferred", (n_users, n_items), d, batches, flush_at=True)
    for n in range(1, lr.STEPS + 1):
        b = [_dev(a) for a in batches[n - 1]]
        losses = [s.step(kind, *b, defer=True).clone() for s in states]
        for k, p in partner.items():
            assert states[k]._seq_lazy is not None and states[p]._seq_lazy is None
            assert torch.equal(losses[k], losses[p]), (n, states[k].lazy_period, losses[k], losses[p])
        if n == lr.FLUSH_AT:
            states[1].flush(); states[4].flush()
            _mf_same(states[4], states[1], "flush after call %d" % n)
        for k, h in zip((2, 3, 4), hists):
            _mf_stamps_are(states[k], [h[0][n], h[1][n]], "call %d" % n)
    for s in states:
        s.flush()
    for k, p in partner.items():
        _mf_same(states[k], states[p], "end")
        _, sp, sq = states[k]._lazy_bufs
        assert int(sp.min()) == lr.STEPS == int(sp.max()) and int(sq.min()) == lr.STEPS == int(sq.max())
    _check_idle_rows(_mf_tables(states), start, lr.STEPS, record_property)


@pytest.mark.parametrize("d", [32, 256])
def test_mf_long_lazy_sequence_ended_by_a_step_that_completes_in_its_call(d):
    """300 calls, the last one without MACR_STEP_DEFER: its own pass and the catch-up of every row (up to 64 steps) run in the call"""
    from macr_amd import ops
    kind_name, n_users, n_items = lr.DEFERRED_SHAPES[d]
    kind, B, steps = getattr(ops, kind_name), lr.DEFERRED_B, 300
    states, _ = _mf_states(n_users, n_items, d, B, [1, 7, 64])
    batches = lr.deferred_batches(d, steps)
    models = [lr.Schedule((n_users, n_items), d, K, "deferred") for K in (7, 64)]
    for n in range(1, steps + 1):
        b = [_dev(a) for a in batches[n - 1]]
        losses = [s.step(kind, *b, defer=n < steps).clone() for s in states]
        for m in models:
            m.step(lr.touched(batches[n - 1]), defer=n < steps)
        assert torch.equal(losses[1], losses[0]) and torch.equal(losses[2], losses[0]), (n, losses)
        if n == steps - 1:                          # what the last call finds: rows from step 256 on (their chunks' last sweep)
            for s, m in zip(states[1:], models):
                _mf_stamps_are(s, [_dev(st.astype(np.int32)) for st in m.stamp], "call %d" % n)
            assert int(models[1].stamp[0].min()) == 256 and int(models[1].stamp[0].max()) == steps - 2
    for s, m in zip(states[1:], models):
        assert s.pending_B == 0 and states[0].pending_B == 0
        _mf_same(s, states[0], "K = %d" % s.lazy_period)
        assert all((st == steps).all() for st in m.stamp)
        _mf_stamps_are(s, [_dev(st.astype(np.int32)) for st in m.stamp], "end")


@pytest.mark.parametrize("d", [32, 256])
def test_mf_lazy_sequence_complete_steps_and_a_new_lazy_sequence(d):
    """270 lazy calls (over the wrap), flush, 5 complete steps (the dense form: they neither tick the counter nor stamp a row),
    70 lazy calls of a new sequence whose ring still holds the first one's steps: the all-dense model bit for bit"""
    from macr_amd import ops
    kind_name, n_users, n_items = lr.DEFERRED_SHAPES[d]
    kind, B, first, complete, second = getattr(ops, kind_name), lr.DEFERRED_B, 270, 5, 70
    states, _ = _mf_states(n_users, n_items, d, B, [1, 7, 64])
    dense, lazies = states[0], states[1:]
    batches = lr.deferred_batches(d, first + complete + second)
    models = [lr.Schedule((n_users, n_items), d, K, "deferred") for K in (7, 64)]
    for n in range(1, len(batches) + 1):
        lazy_call = not first < n <= first + complete
        b = [_dev(a) for a in batches[n - 1]]
        losses = [s.step(kind, *b, defer=lazy_call).clone() for s in states]
        for s, m in zip(lazies, models):
            assert (s._seq_lazy is not None) == lazy_call
            if lazy_call:
                m.step(lr.touched(batches[n - 1]))
        assert torch.equal(losses[1], losses[0]) and torch.equal(losses[2], losses[0]), (n, losses)
        if not lazy_call or n in (first, len(batches)):
            for s, m in zip(states, [None] + models):
                s.flush()
                if m is not None:
                    m.flush()
            for s, m in zip(lazies, models):
                _mf_same(s, dense, "after call %d, K = %d" % (n, s.lazy_period))
                _mf_stamps_are(s, [_dev(st.astype(np.int32)) for st in m.stamp], "after call %d" % n)
    assert all(m.t == first + second and (m.stamp[0] == m.t).all() and (m.stamp[1] == m.t).all() for m in models)
