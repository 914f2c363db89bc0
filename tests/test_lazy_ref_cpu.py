"""tests/lazy_ref.py: the schedule model of the lazy dense Adam pass on cases small enough to check by hand, and the
preconditions (a)-(f) of tests/test_gpu_lazy_adam_horizon.py on exactly the sizes, periods and batches that file runs -- a
long-horizon GPU test that never reached full lag or never crossed the ring's wrap would pass without testing either."""
import os
import re

import numpy as np
import pytest

import lazy_ref as lr
from helpers import REPO


def test_constants_are_the_library_s():
    src = open(os.path.join(REPO, "macr_amd", "csrc", "train_kernels.hip")).read()
    hdr = open(os.path.join(REPO, "include", "macr_hip.h")).read()
    assert int(re.search(r"constexpr int kLazyRing = (\d+);", src).group(1)) == lr.RING
    assert int(re.search(r"#define MACR_LAZY_MAX_PERIOD\s+(\d+)", hdr).group(1)) == lr.MAX_PERIOD
    iters = int(re.search(r"#define MACR_ADAM_ITERS (\d+)", src).group(1))
    assert re.search(r"constexpr int kAdamVecPerBlock = 256 \* kAdamIters;", src)
    for d in (32, 64, 128, 256):
        assert lr.rows_per_chunk(d) == 256 * iters // (d // 4)
    assert [lr.rows_per_chunk(d) for d in (32, 256)] == [128, 16]


def test_sharded_schedule_by_hand():
    """5 rows of d = 256 in one chunk and 40 rows in three, K = 2: chunk c is swept at the steps of its parity"""
    s = lr.Schedule([5, 40], 256, 2, "sharded")
    s.step([[4], [20, 20, 39]])                     # step 1: sweeps the odd chunk (rows 16..31 of table 1)
    assert s.stamp[0].tolist() == [0, 0, 0, 0, 1]
    assert s.stamp[1].tolist() == [0] * 16 + [1] * 16 + [0] * 7 + [1]
    assert s.t == 1 and s.ring[1] == 1 and s.ring[2] == -1
    reads = s.step([[0], [39]])                     # step 2: the even chunks; row 39 (chunk 2) belongs to the sweep, not to a touch block
    assert s.stamp[0].tolist() == [2] * 5 and s.stamp[1].tolist() == [2] * 16 + [1] * 16 + [2] * 8
    by = {(r.reader, r.table): r for r in reads}
    assert by[("touch", 1)].rows.size == 0 and by[("gather", 1)].lag.tolist() == [1] and by[("gather", 1)].span.tolist() == [0]
    assert by[("sweep", 0)].lag.tolist() == [2, 2, 2, 2, 1] and by[("sweep", 0)].span.tolist() == [2, 2, 2, 2, 1]
    s.read_all()
    assert s.stamp[1].tolist() == [2] * 16 + [1] * 16 + [2] * 8      # (nothing written)
    s.flush()
    assert all((st == 2).all() for st in s.stamp)


def test_sharded_schedule_is_the_inline_arithmetic_of_the_existing_test():
    """test_lazy_pass_leaves_untouched_rows_alone_between_sweeps states it as: visited = touched | chunk % K == step % K"""
    n, d, K = 20000, 64, 64
    rs = np.random.RandomState(3)
    s = lr.Schedule([n], d, K, "sharded")
    visited = np.zeros(n, bool)
    chunk_of = np.arange(n) // (1024 // (d // 4))
    for step in range(1, 4):
        u = rs.randint(0, n, 512)
        s.step([u])
        visited[u] = True
        visited |= (chunk_of % K) == (step % K)
    assert np.array_equal(s.stamp[0] != 0, visited)


def test_deferred_schedule_by_hand():
    """one table of 3 chunks (d = 256: 16 rows each), K = 4: stamps run one step behind the counter until the flush"""
    s = lr.Schedule([40], 256, 4, "deferred")
    s.step([[0]])                                   # call 1: nothing pending, nothing moves
    assert s.t == 1 and not s.stamp[0].any() and s.reads == []
    reads = s.step([[17]])                          # call 2: pending step 1 -- rows 0 (its batch), 17 (this batch), chunk 1
    assert s.t == 2 and s.stamp[0].tolist() == [1] + [0] * 15 + [1] * 16 + [0] * 8
    assert [(r.reader, r.rows.tolist(), r.lag.tolist(), r.span.tolist()) for r in reads if r.reader == "fwd"] == [("fwd", [17], [2], [1])]
    s.step([[39]])                                  # call 3: pending step 2 -- rows 17, 39 and chunk 2
    assert s.stamp[0].tolist() == [1] + [0] * 15 + [1, 2] + [1] * 14 + [2] * 8
    s.step([[1]], defer=False)                      # call 4 completes: step 3 (chunk 3: none), then step 4 (chunk 0), then every row
    assert s.t == 4 and (s.stamp[0] == 4).all() and s.pending is None
    s.step([[1]])                                   # a new sequence starts on rows that are all at the counter
    assert s.t == 5 and (s.stamp[0] == 4).all()
    s.flush()
    assert (s.stamp[0] == 5).all()
    assert s.flush() == []                          # (nothing pending: no-op)


def test_model_notices_a_ring_that_is_too_short():
    """the contract lr[s % 256] = step s for s in (t - 256, t]: a row 256 steps behind is served, one 257 behind is not"""
    for K, ok in ((256, True), (257, False)):
        s = lr.Schedule([lr.rows_per_chunk(32) * K], 32, K, "sharded")
        try:
            for _ in range(2 * K + 2):
                s.step([[]])
            assert ok
        except AssertionError as e:
            assert not ok and "asks the ring for step" in str(e)


# ---------------------------------------------------------------------------------------------------------------------
# preconditions of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
def _runs(form, d):
    if form == "sharded":
        sizes, batches = lr.SHARDED_SHAPES[d], lr.sharded_batches(d)
    else:
        sizes, batches = lr.DEFERRED_SHAPES[d][1:], lr.deferred_batches(d)
    out = []
    for k, K in enumerate(lr.PERIODS[1:]):
        flush_at = lr.FLUSH_AT if k == 2 else None
        out.append((K, flush_at) + lr.run_schedule(form, sizes, d, K, batches, flush_at, lr.READ_ALL_AT if form == "sharded" else ()))
    return sizes, batches, out


@pytest.mark.parametrize("form,d", [("sharded", 32), ("sharded", 256), ("deferred", 32), ("deferred", 256)])
def test_preconditions_of_the_horizon_cases(form, d, record_property):
    sizes, batches, runs = _runs(form, d)
    full = 64 if form == "sharded" else 65
    for K, flush_at, hist, stats, sch in runs:
        # (a) the counter passes 256 + 64
        assert sch.t == lr.STEPS >= 256 + 64 + 7
        # (d) no row is ever further behind than the period (+ the pending step); nobody walks more than K ring slots
        assert stats.max_lag <= K + 1 and stats.max_span <= K
        assert stats.max_lag == (K if form == "sharded" else K + 1) and stats.max_span == K
        record_property("K%d%s_max_lag" % (K, "_flushed" if flush_at else ""), stats.max_lag)
        if K != 64:
            continue
        # (b) reads at full lag, by every reader that can be there; (c) some of them across ring slots 255 -> 0
        readers = ("gather", "sweep") if form == "sharded" else ("fwd", "scan")
        for reader in readers:
            assert stats.full.get(reader), (reader, "never at lag %d" % full)
            if not flush_at:
                assert stats.full_straddle.get(reader), (reader, "never across the wrap at lag %d" % full)
                assert all(256 <= s <= 256 + 64 for s in stats.full_straddle[reader])
            record_property("K64%s_%s_full_lag_across_wrap_at" % ("_flushed" if flush_at else "", reader),
                            ",".join(map(str, sorted(set(stats.full_straddle.get(reader, []))))))
        if flush_at:                                 # the flush after step 258 walks stamps from 194 / 195 on, across the wrap
            assert flush_at - 64 <= stats.flush_min <= flush_at - 63 < 255 and all((h[flush_at] == flush_at).all() for h in hist)
            record_property("K64_flush_oldest_stamp", stats.flush_min)
        if form == "deferred":                      # stamps one step behind the counter until the flush
            assert all(int(h[lr.STEPS].max()) == lr.STEPS - 1 for h in hist)
    # (e) the idle rows are never referenced; (f) no row more than 64 times in a batch (deferred: never twice)
    worst = 0
    for b in batches:
        for rows, n in zip(lr.touched(b), sizes):
            assert 0 <= rows.min() and rows.max() < n - lr.IDLE
        worst = max(worst, *lr.max_refs(b))
    assert worst <= 64 if form == "sharded" else worst == 1
    record_property("max_references_of_a_row", worst)
    if form == "sharded":                           # the shapes: fewer chunks than 7 + a partial one; about 70 + a partial one
        rpc = lr.rows_per_chunk(d)
        assert sizes[0] // rpc < 6 and sizes[0] % rpc and 69 <= sizes[1] // rpc <= 71 and sizes[1] % rpc
        assert all(lr.max_refs(b)[1] >= 40 for b in batches)          # the hot runs are there


def test_idle_rows_recurrence_in_fp32_stays_near_the_closed_form():
    """the tolerance input of the GPU test: 330 idle steps in float32 against the fp64 closed form"""
    rs = np.random.RandomState(0)
    theta0 = (rs.standard_normal((lr.IDLE, 32)) * 0.3).astype(np.float32)
    m0, v0 = lr.idle_slots(11, 32)
    (th, m, v), bounds, dev = lr.idle_bounds(theta0, m0, v0, lr.STEPS)
    assert np.array_equal(th[[3, 8]], theta0[[3, 8]].astype(np.float64)) and not m[[3, 8]].any() and not v[[3, 8]].any()
    assert 0 < dev[0] < 5e-6 and np.abs(th - theta0).max() > 1e-3            # the rows move by thousands of those deviations
    # one step by hand: t = 1, lr_1 = lr sqrt(1 - b2) / (1 - b1)
    th1, m1, v1 = lr.idle_closed_form(theta0, m0, v0, 1)
    lr1 = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    np.testing.assert_allclose(th1, theta0 - lr1 * 0.9 * m0.astype(np.float64) / (np.sqrt(0.999 * v0.astype(np.float64)) + 1e-8), rtol=1e-15)
    np.testing.assert_allclose(m1, 0.9 * m0.astype(np.float64), rtol=1e-15)
