"""The schedule of the lazy dense Adam pass (include/macr_hip.h: macr_lazy_adam) as a NumPy model without a single table
value: which row carries which stamp after every step, which step every slot of the lr_t ring holds, and how far behind a
row is whenever something reads it -- for the two forms of the pass,

  sharded   (macr_shard_gather_lazy / macr_shard_apply_lazy: k_rows_gather_owned<LAZY>, k_adam_lazy)   step n:
            the gather reads the batch's rows (counter n - 1), k_shard_keys ticks the counter to n, k_adam_lazy sweeps the
            chunks c with c % K == n % K and updates the first-reference owners outside them: all of them to stamp n.
  deferred  (macr_mf_train_step_lazy with MACR_STEP_DEFER: k_pair_fwd<2>, adam_lazy_scan_block)        call n:
            the pass of step n - 1 is pending: the forward looks from each row's stamp to step n - 1 in registers, the
            blocks riding in the (B,B) launch bring the rows of batch n - 1 (gradient flag), of batch n (marked by the
            forward) and the chunks c % K == (n - 1) % K to stamp n - 1; the backward kernel ticks the counter to n.
            Stamps therefore run one step behind the counter until a flush (or a step that completes in its call).

plus the inputs of tests/test_gpu_lazy_adam_horizon.py (so that tests/test_lazy_ref_cpu.py states their preconditions
without a GPU) and the fp64 / fp32 statements of what an idle row does (part "idle rows" of the horizon tests).

Two figures per read of a row (class Read):
  span  = target - stamp: the ring slots the reader walks, steps stamp + 1 .. target (the gradient step of a pass included);
  lag   = now - stamp, `now` = the step the running call computes (between calls: the counter): how far behind the row is
          for the step that reads it.  Sharded: now = target (passes) or target + 1 (gather).  Deferred: now = target + 1 --
          "a row K steps behind, plus the pending step"."""
import numpy as np

RING = 256                      # kLazyRing (train_kernels.hip)
MAX_PERIOD = 64                 # MACR_LAZY_MAX_PERIOD


def rows_per_chunk(d):
    """rows of d floats in a chunk of kAdamVecPerBlock = 1024 float4 (a row never straddles two chunks)"""
    return 1024 // (d // 4)


class Read(object):
    """one reader's visit to rows of one table: their stamps at that moment, the step they were brought to"""
    __slots__ = ("reader", "table", "rows", "stamps", "target", "counter", "now")

    def __init__(self, reader, table, rows, stamps, target, counter, now):
        self.reader, self.table, self.rows, self.stamps = reader, table, rows, stamps
        self.target, self.counter, self.now = target, counter, now

    @property
    def lag(self):
        return self.now - self.stamps

    @property
    def span(self):
        return self.target - self.stamps

    def straddles(self):
        """rows whose walk stamp + 1 .. target passes from ring slot 255 to slot 0 (steps M - 1 and M, M a multiple of 256)"""
        M = self.target // RING * RING
        return (self.stamps <= M - 2) & (M > 0)


class Schedule(object):
    """stamps (one int64 array per table), counter `t` and ring (slot -> step, -1: never written) of one model.
    step() returns the list of Read of that step; `reads` keeps the last list."""

    def __init__(self, sizes, d, period, form):
        assert form in ("sharded", "deferred") and period >= 1
        self.form, self.K, self.rpc = form, int(period), rows_per_chunk(d)
        self.chunk = [np.arange(n) // self.rpc for n in sizes]
        self.stamp = [np.zeros(n, np.int64) for n in sizes]
        self.t = 0
        self.ring = np.full(RING, -1, np.int64)
        self.ring[0] = 0                                        # "state zero-filled once": slot 0 = step 0, which nobody reads
        self.pending = None                                     # deferred: the rows of the batch whose pass is pending
        self.reads = []

    # ---- the contract of the ring: lr[s % 256] holds step s for s in (t - 256, t]
    def _read(self, reader, table, rows, target, now):
        rows = np.asarray(rows, np.int64)
        st = self.stamp[table][rows].copy()
        if st.size:
            assert target <= self.t and int(st.max()) <= target, (reader, target, self.t, int(st.max()))
            steps = np.arange(int(st.min()) + 1, target + 1)
            bad = steps[self.ring[steps % RING] != steps]
            if bad.size:
                raise AssertionError("%s at counter %d asks the ring for step %d, slot %d holds step %d" % (
                    reader, self.t, bad[0], bad[0] % RING, self.ring[bad[0] % RING]))
        self.reads.append(Read(reader, table, rows, st, target, self.t, now))

    def _tick(self):
        self.t += 1
        self.ring[self.t % RING] = self.t

    def _sweep_rows(self, table, T):
        return np.nonzero(self.chunk[table] % self.K == T % self.K)[0]

    def _all(self, reader, now):
        for tab in range(len(self.stamp)):
            self._read(reader, tab, np.arange(self.stamp[tab].size), self.t, now)

    # ---- sharded form
    def _step_sharded(self, touched):
        now = self.t + 1
        rows = [np.unique(np.asarray(r, np.int64)) for r in touched]
        for tab, r in enumerate(rows):
            self._read("gather", tab, r, self.t, now)
        self._tick()
        T = self.t
        for tab, r in enumerate(rows):
            sweep = self._sweep_rows(tab, T)
            touch = r[self.chunk[tab][r] % self.K != T % self.K]       # (the sweep block owns the others)
            self._read("sweep", tab, sweep, T, now)
            self._read("touch", tab, touch, T, now)
            self.stamp[tab][sweep] = T
            self.stamp[tab][touch] = T

    # ---- deferred form
    def _scan(self, T, flagged, now):
        for tab, r in enumerate(flagged):
            sel = np.union1d(r, self._sweep_rows(tab, T)).astype(np.int64)
            self._read("scan", tab, sel, T, now)
            self.stamp[tab][sel] = T

    def _step_deferred(self, touched, defer):
        now = self.t + 1
        rows = [np.unique(np.asarray(r, np.int64)) for r in touched]
        if self.pending is not None:
            T = self.t                                          # the pending step
            for tab, r in enumerate(rows):
                self._read("fwd", tab, r, T, now)
            self._scan(T, [np.union1d(p, r) for p, r in zip(self.pending, rows)], now)
        else:                                                   # a sequence starts: the forward reads the tables as they are
            for st in self.stamp:
                assert (st == self.t).all(), "a deferred sequence starts on rows that are behind"
        self._tick()
        if defer:
            self.pending = rows
        else:                                                   # the step completes in its call
            self._scan(self.t, rows, now)
            self._flush_all(now)
            self.pending = None

    def _flush_all(self, now):
        self._all("flush", now)
        for st in self.stamp:
            st[:] = self.t

    # ---- what the tests call
    def step(self, touched, defer=True):
        """touched: per table, the rows the step's batch references (any order, repeats allowed)"""
        self.reads = []
        if self.form == "sharded":
            self._step_sharded(touched)
        else:
            self._step_deferred(touched, defer)
        return self.reads

    def read_all(self):
        """macr_lazy_rows over every row of every table, between two steps: nothing changes"""
        self.reads = []
        self._all("rows", self.t)
        return self.reads

    def flush(self):
        self.reads = []
        if self.form == "deferred":
            if self.pending is None:
                return self.reads
            self._scan(self.t, self.pending, self.t)
            self.pending = None
        self._flush_all(self.t)
        return self.reads


class Stats(object):
    """what a run's reads add up to: the preconditions (a)-(d) of the horizon tests"""

    def __init__(self, K):
        self.K, self.max_lag, self.max_span = K, 0, 0
        self.flush_min = None                                   # the oldest stamp the flush of run_schedule met
        self.full, self.full_straddle = {}, {}                  # reader -> the steps (`now`) with a read at full lag / ... across the wrap

    def add(self, reads, full_lag):
        for r in reads:
            if not r.stamps.size:
                continue
            self.max_lag = max(self.max_lag, int(r.lag.max()))
            self.max_span = max(self.max_span, int(r.span.max()))
            full = r.lag == full_lag
            if full.any():
                self.full.setdefault(r.reader, []).append(r.now)
                if (full & r.straddles()).any():
                    self.full_straddle.setdefault(r.reader, []).append(r.now)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the horizon tests
# ---------------------------------------------------------------------------------------------------------------------
STEPS, PERIODS, FLUSH_AT, IDLE, BATCH_SEED = 330, [1, 7, 64, 64], 258, 12, 77
READ_ALL_AT = [s for s in range(1, STEPS + 1) if 250 <= s <= 262 or s % 16 == 0]        # lazy_rows over every row, after step s
SHARDED_B, SHARDED_SHAPES = 96, {32: (300, 8965), 256: (37, 1125)}                     # d -> n_users, n_items
DEFERRED_B, DEFERRED_SHAPES = 128, {32: ("LOSS_RUBIBCEBOTH", 300, 700), 256: ("LOSS_RUBIBCE", 200, 400)}
COLD_CYCLES = (1, 4, 5)         # the sweep cycles (step // 64) in which cold rows are referenced, each row in one of them
SHARDED_COLD = (6, 48)          # sharded: cold rows of the user / item table, below the idle rows


def sharded_batch(rs, n_users, n_items, B, hot=(40, 20)):
    """the draws of tests/test_gpu_lazy_adam.py::_batch, on the host (the GPU test checks that they are the same)"""
    u = rs.choice(n_users, B, replace=B > n_users).astype(np.int32)
    i = rs.randint(0, n_items, B).astype(np.int32)
    i[:hot[0]], i[hot[0]:hot[0] + hot[1]] = 1, 2
    j = rs.randint(3, n_items, B).astype(np.int32)
    return u, i, j


def sharded_batches(d, steps=STEPS, raw=False):
    """batch n = 1 .. steps of the sharded run.  Each table is [rows _batch draws from | COLD rows | IDLE rows]: _batch sees
    the first part only (raw=True: exactly its draws), then the cold rows of the chunk that step n sweeps for K = 64 replace
    the last entries of u / i / j in the cycle n // 64 that is theirs (COLD_CYCLES): each is referenced ONCE, by the gather
    that precedes its chunk's sweep -- 64 steps behind.  (Of the small d = 256 tables _batch references every row every
    few steps: without the cold rows no gather would ever meet a row at full lag.)"""
    n_users, n_items = SHARDED_SHAPES[d]
    rpc, B = rows_per_chunk(d), SHARDED_B
    cold = [np.arange(n - IDLE - c, n - IDLE) for n, c in zip((n_users, n_items), SHARDED_COLD)]
    rs = np.random.RandomState(BATCH_SEED)
    out = []
    for n in range(1, steps + 1):
        u, i, j = sharded_batch(rs, cold[0][0], cold[1][0], B)
        cyc, phase = divmod(n, MAX_PERIOD)
        if cyc in COLD_CYCLES and not raw:
            for tab, rows in enumerate(cold):
                mine = rows[(rows // rpc % MAX_PERIOD == phase) & ((rows - rows[0]) % len(COLD_CYCLES) == COLD_CYCLES.index(cyc))]
                for k, r in enumerate(mine):
                    (u if tab == 0 else i if k % 2 else j)[B - 1 - k] = r
        out.append((u, i, j))
    return out


def cold_rows(n_rows, d):
    """(chunks, len(COLD_CYCLES)) rows: the first rows of every chunk that lie wholly below the idle rows"""
    rpc = rows_per_chunk(d)
    starts = np.arange(0, n_rows - IDLE - len(COLD_CYCLES) + 1, rpc)
    return starts[:, None] + np.arange(len(COLD_CYCLES))[None, :]


def deferred_batches(d, steps=STEPS):
    """batch n = 1 .. steps of the deferred run: no row twice in a batch, none of the last IDLE rows, and COLD rows that the
    random draws leave out: the k-th cold row of chunk c is referenced ONCE, in call n with n - 1 = 64 * COLD_CYCLES[k] + c --
    the call whose pending step n - 1 sweeps chunk c for K = 64, so the forward meets the row 64 steps behind the pending
    step (65 behind its own).  Random rows are referenced every few steps and would never get there."""
    _, n_users, n_items = DEFERRED_SHAPES[d]
    B = DEFERRED_B
    cu, ci = cold_rows(n_users, d), cold_rows(n_items, d)
    pool_u = np.setdiff1d(np.arange(n_users - IDLE), cu.ravel())
    pool_i = np.setdiff1d(np.arange(n_items - IDLE), ci.ravel())
    rs = np.random.RandomState(BATCH_SEED + d)
    out = []
    for n in range(1, steps + 1):
        u = rs.choice(pool_u, B, replace=False).astype(np.int32)
        ij = rs.choice(pool_i, 2 * B, replace=False).astype(np.int32)
        i, j = ij[:B].copy(), ij[B:].copy()
        cyc, c = divmod(n - 1, MAX_PERIOD)
        if cyc in COLD_CYCLES:
            k = COLD_CYCLES.index(cyc)
            if c < len(cu):
                u[0] = cu[c, k]
            if c < len(ci):
                (i if c % 2 else j)[1] = ci[c, k]               # as the positive or as the negative item
        out.append((u, i, j))
    return out


def touched(batch):
    u, i, j = batch
    return [u, np.concatenate([i, j])]


def max_refs(batch):
    """the most references one row has in the batch (user rows, item rows)"""
    u, i, j = batch
    return int(np.bincount(u).max()), int(np.bincount(np.concatenate([i, j])).max())


def run_schedule(form, sizes, d, K, batches, flush_at=None, read_all_at=()):
    """the whole run of one model: (stamps after every step: per table an (steps + 1, n) array, Stats, the Schedule).
    flush_at: a flush after that step.  Full lag: K (sharded), K + 1 (deferred)."""
    sch, stats = Schedule(sizes, d, K, form), Stats(K)
    full = K if form == "sharded" else K + 1
    hist = [np.zeros((len(batches) + 1, n), np.int64) for n in sizes]
    for n, b in enumerate(batches, 1):
        stats.add(sch.step(touched(b)), full)
        if n in read_all_at:
            stats.add(sch.read_all(), full)
        if n == flush_at:
            stats.add(sch.flush(), full)
            stats.flush_min = min(int(r.stamps.min()) for r in sch.reads if r.stamps.size)
        for tab in range(len(sizes)):
            hist[tab][n] = sch.stamp[tab]
    return hist, stats, sch


# ---------------------------------------------------------------------------------------------------------------------
# a row no batch references: m_T = b1^T m_0, v_T = b2^T v_0, theta_T = theta_0 - sum_t lr_t b1^t m_0 / (sqrt(b2^t v_0) + eps)
# ---------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8        # make_hyper(1e-3, ...) of the tests: tf.train.AdamOptimizer's defaults


def idle_slots(seed, d, n=IDLE):
    """Adam slots to put under the idle rows before the first step: m ~ N(0, 1e-3), v = |N(0, 1)| 1e-5, rows 3 and 8 zero"""
    rs = np.random.RandomState(seed)
    m = (rs.standard_normal((n, d)) * 1e-3).astype(np.float32)
    v = (np.abs(rs.standard_normal((n, d))) * 1e-5).astype(np.float32)
    m[[3, 8]] = 0
    v[[3, 8]] = 0
    return m, v


def idle_closed_form(theta0, m0, v0, T):
    th, m0, v0 = (np.asarray(a, np.float64).copy() for a in (theta0, m0, v0))
    for t in range(1, T + 1):
        lr_t = LR * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
        th -= lr_t * (B1 ** t * m0) / (np.sqrt(B2 ** t * v0) + EPS)
    return th, B1 ** T * m0, B2 ** T * v0


def idle_fp32(theta0, m0, v0, T):
    """the same T steps one by one in float32, every operation rounded on its own: the arithmetic of the oracle's Adam pass
    (orc_adam_lr_t, orc_adam_dense with g = 0; the beta powers are fp32 state multiplied once per step)"""
    f = np.float32
    th, m, v = (np.asarray(a, f).copy() for a in (theta0, m0, v0))
    lr, b1, b2, eps, p1, p2 = f(LR), f(B1), f(B2), f(EPS), f(B1), f(B2)
    for _ in range(T):
        lr_t = f(f(lr * f(np.sqrt(f(f(1) - p2)))) / f(f(1) - p1))
        p1, p2 = f(p1 * b1), f(p2 * b2)
        m = m * b1
        v = v * b2
        th = th - (lr_t * m) / (np.sqrt(v) + eps)
    assert th.dtype == f and m.dtype == f and v.dtype == f
    return th, m, v


def idle_bounds(theta0, m0, v0, T):
    """(closed form (theta, m, v) in fp64, bounds, CPU deviations): bound = 4 x the largest deviation of the float32 run
    from the closed form over these rows + one float32 ulp of the value"""
    want = idle_closed_form(theta0, m0, v0, T)
    got = idle_fp32(theta0, m0, v0, T)
    dev = [float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want)]
    bounds = [4.0 * e + np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) for e, w in zip(dev, want)]
    return want, bounds, dev
