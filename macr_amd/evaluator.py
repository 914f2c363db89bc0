"""Full-catalogue top-K evaluator on the HIP path.

Replaces the per-batch  sess.run(ratings) -> host  -> per-user Python/C++ ranking
of the reference:
  * macr_mf/train.py  test() :162-311  (+ test_one_user :119-138, metrics :32-117)
  * macr_lightgcn/utility/batch_test.py  test() :26-162  (+ evaluator/cpp)
with: branch sigmoids -> fused scoring/mask/top-K (MFMA) -> merge of splits ->
[multi-GPU: one RCCL all-gather of the per-shard top-K + merge] -> metrics
kernel -> column means.  Nothing U x N ever leaves the device (or exists).

Both reference evaluators batch the users by BATCH_SIZE; every per-user result
is independent of the batching, so all query users are ranked in one pass.

Three parts: WHAT the next evaluation tries (seeds or a sampling pass, which candidate filter) is eval_policy.py's
state machine, replaced -- never mutated -- in `self._policy`; HOW a ranking is launched travels as arguments
(rank_local: seeded, mode, repair_of, filter), and the same arguments are the graph-cache key; the graph cache itself
is _captured / _replay.
"""
import os

import numpy as np
import torch

from . import _lib, eval_policy, ops, sharding


class Ranked(tuple):
    """(vals, idx) of rank_local, and `.seeded`: the ranking took its thresholds from the previous one's candidates"""
    def __new__(cls, vals, idx, seeded):
        self = tuple.__new__(cls, (vals, idx))
        self.seeded = seeded
        return self


def _ptrs(*tensors):
    return tuple(None if t is None else t.data_ptr() for t in tensors)


class Evaluator(object):
    def __init__(self, mask_lists, gt_lists, n_items, device):
        """mask_lists[q]: the train items of query user q (excluded from ranking, train.py:132-133 /
        batch_test.py:124-129); gt_lists[q]: its test (or valid) items."""
        assert len(mask_lists) == len(gt_lists)
        self.n_queries = len(gt_lists)
        self.n_items = n_items
        device = torch.device(device)
        self.device = device
        self.mask = ops.CSR.from_lists(mask_lists, device)
        self.max_queries_per_pass = 131072       # bounds the ranking workspace (~1.5 GB of candidate lists)
        self.use_graph = os.environ.get("MACR_EVAL_GRAPH", "1") != "0"    # replay the evaluation as one HIP graph (_means)
        self.use_seeds = os.environ.get("MACR_EVAL_SEEDS", "1") != "0"    # thresholds from the previous top K (rank_local)
        # candidate filter of the listing pass, an argument of every ranking call (include/macr_hip.h MACR_EVAL_FILTER_*): "f16" (default, round 6) =
        # one fp16 number per operand on the fp16 matrix cores, "bf16" = two-term bf16 products on the bf16 matrix cores -- both
        # with fp32 re-scoring of the best candidates -- "f32" = fp32 products throughout.  The ranking is the fp32 ranking bit
        # for bit whichever it is; MACR_EVAL_FILTER in the environment overrides the default; the policy (eval_policy.py) steps
        # down f16 -> bf16 -> f32 where a model's scores are packed closer than a filter resolves.
        self.filter = os.environ.get("MACR_EVAL_FILTER", "f16").strip().lower()
        ops.eval_filter_code(self.filter)         # a typo in the environment is refused here, by name
        # One GPU, graph replays: an evaluation launches the FIRST ROUND of the ranking only and writes its means and the
        # ranking's stats straight into pinned host memory; the host, which waits for the means anyway, sees whether a
        # candidate list overflowed or the seeds were stale and, in that rare case, replays the REST of the ranking (repair
        # round, fallback: macr_score_topk_repair_round) on the same workspace and outputs.  Saves the launches that find
        # nothing to do (~25 us of a 0.45 ms evaluation on the Gowalla shape) and both result copies.
        # MACR_EVAL_OPTIMISTIC=0: the complete sequence always.
        self.optimistic = os.environ.get("MACR_EVAL_OPTIMISTIC", "1") != "0"
        # Launch folds.  "p" (default): the branch factors and the ranking's workspace initialisation are one launch
        # (macr_score_topk_prologue): -6 .. -8 us per graph-replayed evaluation on the Gowalla shape, same box.  "m": the
        # MF metrics and their means as one launch (macr_metrics_mf_mean): 20 us against 12.6 + 7.5 us for the two kernels it
        # replaces -- no gain under graph replay (profiles/r05_eval_fold_ab.txt), so off unless asked for.  "1": both, "0": none.
        fold = os.environ.get("MACR_EVAL_FOLD", "p").strip().lower()
        self.fold_prologue, self.fold_metrics = fold in ("1", "p"), fold in ("1", "m")
        self.fold_prep = os.environ.get("MACR_EVAL_FOLD_PREP", "1") != "0"       # (A/B switch of macr_score_topk_prologue_prep)
        self._policy = eval_policy.State()        # seed / filter back-offs: _seed_skip ... _bf16_backoff below read and replace it
        self.fast_stats = {"fast": 0, "redone": 0}
        self._last_info = None
        self._graphs = {}
        self._graph_misses = 0
        self._graph_misses_by_shape = {}
        self._host_out = {}                       # (flavour, Ks) -> pinned means of the first-round path
        self._seeds = {}                          # _seed_key -> (U, SEED_WIDTH) ids the last ranking of that shard left
        self._uses_seeds = {}                     # _shape_uses_seeds
        self._mean_ws = {}                        # len(Ks) -> scratch of macr_metrics_mf_mean
        self._c_sweep = {}                        # group size -> the device array of a sweep's values of c
        self._c_dev = torch.zeros(1, dtype=torch.float32, device=device)         # _c_scalar
        self._c_host = None
        self._stats = torch.zeros(2, dtype=torch.int32, device=device)          # macr_score_topk stats of the last ranking
        self._stats_host = torch.zeros(2, dtype=torch.int32)
        self._stats_first = torch.zeros(2, dtype=torch.int32)          # written by the first-round ranking's own kernel
        if device.type == "cuda":
            self._stats_host = self._stats_host.pin_memory()
            self._stats_first = self._stats_first.pin_memory()
        self._stats_evt = None
        self._last_seeded = False
        self.gt = ops.CSR.from_lists(gt_lists, device)
        self.n_gt = sum(len(row) for row in gt_lists)            # (gt.idx holds one padding element when this is 0)
        # (lo, hi): the `items_tab` the methods below receive is ALREADY this rank's shard, rows [lo, hi) of a catalogue
        # whose full table exists nowhere (row-sharded training, BASELINE configs[4]); None: a replicated full table
        self.local_items_range = None
        # the same for a STRIDED shard (set_local_items): local row l is item lo + l * stride
        self._local_own = None
        self._mask_lists = mask_lists
        self._gt_lists = gt_lists
        self._base = None                         # (shard it was built for, the evaluator list_shift ranks the base with)

    def set_local_items(self, own):
        """`items_tab` is this rank's shard of an item table sharded like the training state (sharded_train.Owned: local
        row l = item own.lo + l * own.stride).  A contiguous shard is an item offset; an interleaved one is ranked in LOCAL
        ids against the owned part of every query's train list and its ids are mapped back before the shards meet."""
        if own.stride == 1:
            self.local_items_range = (own.lo, own.lo + own.n)
            self._local_own = None
            return
        self.local_items_range = None
        self._local_own = own
        local_lists = [[(g - own.lo) // own.stride for g in row if g >= own.lo and (g - own.lo) % own.stride == 0
                        and (g - own.lo) // own.stride < own.n] for row in self._mask_lists]
        self._mask_local = ops.CSR.from_lists(local_lists, self.device)
        self._seeds = {}

    def _shard_range(self, n_rows):
        """(lo, hi) of this rank's item rows, given the rows of the table the caller holds"""
        if self._local_own is not None:
            return 0, self._local_own.n
        if self.local_items_range is not None:
            return tuple(self.local_items_range)
        return sharding.item_shard_range(n_rows, *sharding.world())

    def _shard(self, items_tab):
        """(lo, hi, this rank's rows of the item table)"""
        lo, hi = self._shard_range(items_tab.shape[0])
        if self._local_own is not None or self.local_items_range is not None:
            assert items_tab.shape[0] == hi - lo
            return lo, hi, items_tab
        return lo, hi, items_tab[lo:hi]

    # ------------------------------------------------------------------ ranking
    def rank_local(self, kind, users_tab, user_ids, items_tab, K, w=None, wu=None, c=0.0, branch=None, *,
                   seeded=True, mode=None, repair_of=None, filter=None):
        """This rank's item shard: Ranked (val, idx) of shape (U,K) with GLOBAL item ids.
        users_tab/items_tab: full embedding tables (replicated on every rank); a rank scores only its contiguous
        item shard.  branch (None: items_tab): the table, shaped and sharded like items_tab, the items' branch factors
        sigmoid(row . w) come from (LightGCN's rubi_ratings2: the ego item rows).
        seeded: take the thresholds from the seeds, if there are any; mode: None = the complete ranking, "first" / "repair" =
        its two halves (repair_of: the first round's outputs and workspace); filter: None = filter_now."""
        ws = sharding.world()[1]
        self._last_depth = K
        lo, hi, items_local = self._shard(items_tab)
        branch_local = items_local if branch is None else self._shard(branch)[2]
        filter = filter or self.filter_now
        sig_u = sig_i = None
        U = self.n_queries
        both = kind in (ops.SCORE_RUBI_BOTH, ops.SCORE_DIRECT_MINUS_BOTH)
        mask = self._mask_local if self._local_own is not None else self.mask
        # one ranking call that initialises its own workspace: the branch factors and that initialisation are ONE launch
        # (macr_score_topk_prologue, below, once it is known whether the call is seeded)
        fold = (kind != ops.SCORE_NORMAL and U <= self.max_queries_per_pass and mode != "repair"
                and items_local.shape[1] == users_tab.shape[1] and self.fold_prologue)
        if fold:
            pass
        elif both and items_local.shape[1] == users_tab.shape[1]:
            # sigmoid(e_i . w), sigmoid(e_u . w_user) (model.py:141-142,:199-201) in one launch
            sig_i, sig_u = ops.branch_sigmoid2(branch_local, w, None, users_tab, wu, user_ids)
        elif kind != ops.SCORE_NORMAL:
            sig_i = ops.branch_sigmoid(branch_local, w)             # sigmoid(e_i . w)      model.py:141-142,:199-201
            if both:
                sig_u = ops.branch_sigmoid(users_tab, wu, user_ids)     # sigmoid(e_u . w_user) model.py:199,:201
        if U <= self.max_queries_per_pass:
            # Seeds: the ids this shard returned last time (same queries, tables that moved by a few training steps).
            # Their exact current scores bound every query's K-th best score from below far more tightly than a
            # sampling pass does, for a tenth of its time (k_tau_seed); the ranking itself does not depend on them.
            # Seeds the tables have moved away from (early epochs) cost a repair round, so the policy watches how
            # many query blocks were listed twice (eval_policy.py) and goes back to the sampling pass for a while.
            thresholds = K <= _lib.MAX_TOPK_FUSED and self._shape_uses_seeds(hi - lo, items_tab.shape[1])
            use = self.use_seeds and ws == 1 and thresholds       # (the wide ranking takes no seeds)
            skey = self._seed_key(K, lo, hi, branch)
            seed = self._seeds.get(skey) if use else None
            seeded = seed is not None and seeded
            if use and seed is None:
                seed = self._seeds[skey] = torch.full((U, ops.SEED_WIDTH), -1, dtype=torch.int32, device=self.device)
            # the ranking leaves its best SEED_WIDTH candidates per query in `seed` (in place): the next ranking's seeds
            # under the fp16 filter the prologue also writes the listing pass's operand copies: every row read once (the tables are
            # cold after a log interval of training) -- not for a catalogue small enough to list everything, which runs no filter
            fold_prep = fold and self.fold_prep and filter == "f16" and thresholds
            if fold_prep:
                sig_i, sig_u = ops.score_topk_prologue_prep(kind, users_tab, user_ids, items_local, K, w, wu if both else None, c,
                                                            seeded_first_round=seeded and mode == "first",
                                                            item_branch=None if branch is None else branch_local)
            elif fold:
                # (the prologue reads its item rows for the branch factors only: the branch table stands there)
                sig_i, sig_u = ops.score_topk_prologue(users_tab, user_ids, branch_local, K, w, wu if both else None,
                                                       seeded_first_round=seeded and mode == "first", filter=filter)
            vals, idx = ops.score_topk(kind, users_tab, user_ids, items_local, K, sig_u, sig_i, c, mask, lo,
                                       seed=seed if seeded else None, seed_out=seed,
                                       stats=self._stats_first if mode else self._stats, first_round=mode == "first",
                                       repair_of=repair_of if mode == "repair" else None, filter=filter,
                                       ws_ready=fold, prep_ready=fold_prep)
        else:
            # the ranking workspace (candidate lists, mask bitmap) grows with the number of queries: rank them in
            # chunks; every query is independent of the chunking
            seeded, parts = False, []
            for a in range(0, U, self.max_queries_per_pass):
                b = min(U, a + self.max_queries_per_pass)
                uid = user_ids[a:b] if user_ids is not None else torch.arange(a, b, dtype=torch.int32, device=self.device)
                parts.append(ops.score_topk(kind, users_tab, uid, items_local, K, None if sig_u is None else sig_u[a:b],
                                            sig_i, c, mask.row_range(a, b), lo, filter=filter))
            vals = torch.cat([p[0] for p in parts], dim=1)
            idx = torch.cat([p[1] for p in parts], dim=1)
        if self._local_own is not None:           # local row -> item id (the order by id within the shard is the same either way)
            own = self._local_own
            idx = torch.where(idx >= 0, idx * own.stride + own.lo, idx)
        return Ranked(vals, idx, seeded)

    def _seed_feedback(self):
        """Complete path: whether the ranking about to be launched takes its thresholds from the seeds
        (eval_policy.seed_complete), once the previous seeded ranking's stats -- if a copy is in flight -- have been read.
        The choice only moves time around: every mode returns the same ranking."""
        world = sharding.world()[1]
        relisted = None
        if self._stats_evt is not None and eval_policy.seeds_allowed(self.use_seeds, world):
            self._stats_evt.synchronize()         # normally long complete: the caller has read the previous metrics
            self._stats_evt = None
            if self._last_seeded:
                relisted = int(self._stats_host[0])
        seeded, self._policy = eval_policy.seed_complete(self._policy, self.use_seeds, world, relisted,
                                                         eval_policy.relist_tolerance(self.n_queries))
        return seeded

    @property
    def filter_now(self):
        """the candidate filter of the ranking about to be launched: `filter`, or "f32" while a reduced-precision filter
        ("bf16", "f16") is backed off"""
        return eval_policy.filter_now(self.filter, self._policy)

    def _shape_uses_seeds(self, n_local, d):
        """False for shards small enough that the ranking lists every unmasked item (no thresholds to seed)"""
        key = (n_local, d)
        if key not in self._uses_seeds:
            self._uses_seeds[key] = bool(_lib.lib().macr_score_topk_uses_seeds(self.n_queries, n_local, d))
        return self._uses_seeds[key]

    @staticmethod
    def _seed_key(K, lo, hi, branch):
        return (K, lo, hi) + (() if branch is None else (branch.data_ptr(),))       # (rubi1 and rubi2 rank differently)

    def _has_seeds(self, K, n_items, branch=None):
        return self._seed_key(K, *self._shard_range(n_items), branch) in self._seeds

    def _stats_readback(self, seeded):
        """after a ranking was launched: its stats travel to the host behind it (no synchronisation here)"""
        self._last_seeded = seeded
        if seeded and self.device.type == "cuda":           # only a seeded ranking's stats steer anything
            self._stats_host.copy_(self._stats, non_blocking=True)
            self._stats_evt = torch.cuda.Event()
            self._stats_evt.record()

    def rank(self, kind, users_tab, user_ids, items_tab, K, w=None, wu=None, c=0.0, fill_masked=False, branch=None):
        """Top-K item ids for every query user: (val (U,K), idx (U,K), cnt (U,)); the shards' top-K are all-gathered
        (one collective) and merged."""
        ranked = self.rank_local(kind, users_tab, user_ids, items_tab, K, w, wu, c, branch, seeded=self._seed_feedback())
        self._stats_readback(ranked.seeded)
        vals, idx = ranked
        fill = self.mask if fill_masked else None
        if sharding.world()[1] == 1:
            return ops.topk_merge(vals, idx, fill)
        lv, li, _ = ops.topk_merge(vals, idx)                        # merge this shard's splits
        gv, gi = sharding.gather_topk(lv, li)                        # (W,U,K) over RCCL / xGMI
        return ops.topk_merge(gv, gi, fill)

    def _groups_on_device(self, group_of, n_groups):
        """(int32 device tensor of the items' group ids or None, n_groups; None: max + 1)"""
        if group_of is None:
            return None, n_groups
        group_of = torch.as_tensor(np.asarray(group_of.cpu() if torch.is_tensor(group_of) else group_of), dtype=torch.int32)
        if n_groups is None:
            n_groups = int(group_of.max()) + 1
        return group_of.to(self.device).contiguous(), n_groups

    # ------------------------------------------------------------------ per-item diagnostic (--out 1)
    def item_accuracy(self, kind, users_tab, user_ids, items_tab, k, w=None, wu=None, c=0.0, branch=None, group_of=None,
                      n_groups=None):
        """The counts behind the reference's item_acc_list (macr_mf/train.py:261-277, k = 5; batch_test.py:94-115,
        k = 20) for the ranking an evaluation with the same arguments scores: (rec_cnt, hit_cnt, group_sums) --
        int32[n_items] users whose k best non-train items contain the item / those of them whose ground truth holds it,
        and with group_of (n_items group ids, 0 .. n_groups-1; n_groups None: max + 1) the int64 (n_groups, 2) sums per
        group, else None.  Ranked by rank() without the -inf fill, at the depth of the evaluator's last ranking when that
        is deeper than k (one set of seeds serves both); counted on the MERGED ranking, which every rank holds after
        rank()'s all-gather: correct under item sharding without a collective of its own."""
        depth = max(int(k), getattr(self, "_last_depth", 0))
        _, idx, _ = self.rank(kind, users_tab, user_ids, items_tab, depth, w, wu, c, fill_masked=False, branch=branch)
        group_of, n_groups = self._groups_on_device(group_of, n_groups)
        return ops.item_counts(idx, self.gt, k, self.n_items, group_of, n_groups or 0)

    # ------------------------------------------------------------------ exposure report (MACR_EXPOSURE_REPORT=1)
    def item_exposure(self, kind, users_tab, user_ids, items_tab, k, w=None, wu=None, c=0.0, branch=None, group_of=None,
                      n_groups=None):
        """What exposure.summarize needs of the ranking an evaluation with the same arguments scores:
        (rec_cnt, exp_w, hit_w, group_sums) on the device -- int32[n_items] users whose k best non-train items contain the
        item (item_accuracy's rec_cnt), int64[n_items] the sum of exposure.position_weights(k)[p] over those list entries
        and over the hits among them, and with group_of (n_items group ids, 0 .. n_groups-1; n_groups None: max + 1) the
        int64 (n_groups, 2) {exp, hit} sums per group, else None.  Ranked as item_accuracy ranks (rank() without the -inf
        fill, at the evaluator's last depth when that is deeper than k) and counted on the MERGED ranking, which every
        rank holds after rank()'s all-gather: correct under item sharding (several ranks, set_local_items) without a
        collective of its own.  Integer sums: the same bytes for every number of ranks."""
        from . import exposure
        depth = max(int(k), getattr(self, "_last_depth", 0))
        _, idx, _ = self.rank(kind, users_tab, user_ids, items_tab, depth, w, wu, c, fill_masked=False, branch=branch)
        group_of, n_groups = self._groups_on_device(group_of, n_groups)
        rec, _, _ = ops.item_counts(idx, self.gt, k, self.n_items)
        exp_w, hit_w, sums = ops.item_exposure(idx, self.gt, exposure.position_weights(k), self.n_items, group_of, n_groups or 0)
        return rec, exp_w, hit_w, sums

    # ------------------------------------------------------------------ list shift report (MACR_SHIFT_REPORT)
    def _base_evaluator(self):
        """The evaluator list_shift ranks the base with: the same lists and item shard as this one, seeds, policy counters and
        graph cache of its own -- a second ranking of another score kind leaves this evaluator's state as it was."""
        shard = (self._local_own, None if self.local_items_range is None else tuple(self.local_items_range))
        if self._base is None or self._base[0] != shard:
            ev = Evaluator(self._mask_lists, self._gt_lists, self.n_items, self.device)
            if self._local_own is not None:
                ev.set_local_items(self._local_own)
            elif self.local_items_range is not None:
                ev.local_items_range = tuple(self.local_items_range)
            self._base = (shard, ev)
        return self._base[1]

    def list_shift(self, kind, users_tab, user_ids, items_tab, k, w=None, wu=None, c=0.0, branch=None,
                   base_kind=ops.SCORE_NORMAL, base_c=0.0, group_of=None, n_groups=None):
        """What the correction changed, query by query: the top-k ranking an evaluation with the same arguments scores
        ("here") against the top-k ranking by base_kind / base_c ("base", default: the factual ranking --test normal prints).
        -> (per_user, entered, left, entered_counts, left_counts) on the device: int32 (U,8) {n_base, n_here, common,
        first_diff, footrule, hits_base, hits_here, hits_common} and int32 (U,k) the ids that entered / left each list,
        ascending, then -1 (ops.list_shift), and ops.item_counts of the entered and of the left lists: (rec_cnt, hit_cnt,
        group_sums) -- how often an item entered (left) a list, how often as a gained (lost) hit, and with group_of (n_items
        group ids, 0 .. n_groups-1; n_groups None: max + 1) the int64 (n_groups, 2) sums per group, else None.
        Both are ranked as item_exposure ranks (rank() without the -inf fill, `here` at the evaluator's last depth when that
        is deeper than k) and compared on the MERGED rankings, which every rank holds after rank()'s all-gather: correct under
        item sharding (several ranks, set_local_items) without a collective of its own.  The base is ranked by an evaluator
        of its own (_base_evaluator)."""
        k = int(k)
        depth = max(k, getattr(self, "_last_depth", 0))
        _, here, _ = self.rank(kind, users_tab, user_ids, items_tab, depth, w, wu, c, fill_masked=False, branch=branch)
        _, base, _ = self._base_evaluator().rank(base_kind, users_tab, user_ids, items_tab, k, w, wu, base_c, fill_masked=False,
                                                 branch=branch)
        per_user, entered, left = ops.list_shift(base, here, self.gt, k, self.n_items)
        group_of, n_groups = self._groups_on_device(group_of, n_groups)
        counts = tuple(ops.item_counts(ids, self.gt, k, self.n_items, group_of, n_groups or 0) for ids in (entered, left))
        return per_user, entered, left, counts[0], counts[1]

    # ------------------------------------------------------------------ calibration report (MACR_CALIBRATION_REPORT)
    def list_calibration(self, kind, users_tab, user_ids, items_tab, k, w=None, wu=None, c=0.0, branch=None, group_of=None,
                         n_groups=None, item_weight=None, with_base=False):
        """The popularity mix of every query user's profile and of its list, for calibration.summarize:
        (profile, here, base) on the device.  profile = (cnt, wsum) of the user's train list (the mask CSR, global ids):
        int32 (U, n_groups) train items per group and int64 (U,2) {sum of item_weight, train items}; computed once per
        evaluator and (group_of, n_groups, item_weight) and kept -- train lists never change.  here = (cnt, hit, wsum) of
        the first k slots of the ranking an evaluation with the same arguments scores: list entries per group, those of
        them in the user's ground truth, {sum of item_weight, list entries} (ops.group_hist).  base: the same triple for
        the factual ranking (SCORE_NORMAL) with with_base, ranked by an evaluator of its own (_base_evaluator: this one's
        seeds, policy state and graph cache stay as they were); else None.  group_of: n_items group ids, 0 .. n_groups-1
        (n_groups None: max + 1); item_weight: n_items integers below 2^31 (the train counts) or None.
        Ranked as item_exposure ranks (rank() without the -inf fill, `here` at the evaluator's last depth when that is
        deeper than k) and counted on the MERGED rankings and the global-id train lists, which every rank holds: the same
        bytes on one rank, on several and under item sharding, without a collective of its own."""
        if group_of is None:
            raise _lib.MacrError(_lib.E_INVALID, "list_calibration: group_of (one group id per item) is required")
        k = int(k)
        host = lambda a: None if a is None else np.asarray(a.cpu() if torch.is_tensor(a) else a).astype(np.int32)
        group_of, item_weight = host(group_of), host(item_weight)
        key = (group_of.tobytes(), n_groups, None if item_weight is None else item_weight.tobytes())
        cached = getattr(self, "_calibration", None)
        if cached is None or cached[0] != key:
            groups, n = self._groups_on_device(group_of, n_groups)
            weight = None if item_weight is None else self._groups_on_device(item_weight, 0)[0]
            cnt, _, wsum = ops.group_hist(self.mask, groups, n, self.n_items, item_weight=weight)
            cached = self._calibration = (key, groups, n, weight, (cnt, wsum))
        _, groups, n, weight, profile = cached
        depth = max(k, getattr(self, "_last_depth", 0))
        _, here, _ = self.rank(kind, users_tab, user_ids, items_tab, depth, w, wu, c, fill_masked=False, branch=branch)
        lists = [here]
        if with_base:
            lists.append(self._base_evaluator().rank(ops.SCORE_NORMAL, users_tab, user_ids, items_tab, k, w, wu, 0.0,
                                                     fill_masked=False, branch=branch)[1])
        out = [ops.group_hist(ids, groups, n, self.n_items, k=k, gt=self.gt, item_weight=weight) for ids in lists]
        return profile, out[0], (out[1] if with_base else None)

    @staticmethod
    def _pairs_of(ids):
        """(ptr, idx, n_pairs): the non-negative entries of an (U,k) id array, row by row, as the pair CSR of rank_positions"""
        valid = ids >= 0
        ptr = torch.zeros(ids.shape[0] + 1, dtype=torch.int32, device=ids.device)
        ptr[1:] = torch.cumsum(valid.sum(dim=1), 0)
        idx = ids[valid].contiguous()
        n_pairs = int(idx.numel())
        return ptr, (idx if n_pairs else torch.zeros(1, dtype=torch.int32, device=ids.device)), n_pairs

    def shift_depth(self, kind, users_tab, user_ids, items_tab, entered, left, w=None, wu=None, c=0.0, branch=None,
                    base_kind=ops.SCORE_NORMAL, base_c=0.0):
        """(pos_entered, pos_left): int32 on the device, one per non-negative entry of list_shift's `entered` / `left` read
        row-major -- the exact 0-based position of every entered item in the full BASE ranking (how deep the correction
        reached for it) and of every left item in the full ranking by kind / c (how far it fell); -1 as rank_positions
        gives it.  A whole, replicated item table on one rank only (rank_positions' NotImplementedError otherwise)."""
        pos_entered = self.rank_positions(base_kind, users_tab, user_ids, items_tab, w, wu, base_c, branch, pairs=self._pairs_of(entered))
        pos_left = self.rank_positions(kind, users_tab, user_ids, items_tab, w, wu, c, branch, pairs=self._pairs_of(left))
        return pos_entered, pos_left

    # ------------------------------------------------------------------ full-catalogue positions (MACR_RANK_REPORT=1)
    def rank_positions(self, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None, pairs=None):
        """int32[n_gt] on the device, in the order of the ground-truth CSR: for every held-out (query, item) pair the number
        of the query's candidates -- the catalogue minus its train items -- ranked before the item by the score an
        evaluation with the same arguments ranks by (score descending, ties by ascending id): the index rank() would
        give the item with K large enough, wherever it stands.  -1: the item is also a train item of the query, or scores
        NaN.  The branch factors are computed as rank() computes them (branch: the ego item rows of LightGCN's rubi2).
        One item shard only (NotImplementedError otherwise): rank_positions_sharded adds the counts of several shards.
        pairs: optional (ptr, idx, n_pairs) CSR over the queries, device int32, ascending per query, in place of the ground
        truth -- int32[n_pairs] in its order (shift_depth: the items that entered or left a list)."""
        if sharding.world()[1] > 1 or self._local_own is not None or self.local_items_range is not None:
            raise NotImplementedError("Evaluator.rank_positions ranks a whole, replicated item table: item-sharded "
                                      "evaluation (several ranks, set_local_items) has no position count yet")
        if items_tab.shape[0] != self.n_items:
            raise _lib.MacrError(_lib.E_INVALID, "rank_positions: %d item rows for an evaluator of %d items" % (items_tab.shape[0], self.n_items))
        sig_u, sig_i = self._branch_factors(kind, users_tab, user_ids, items_tab if branch is None else branch, w, wu)
        csr, n_pairs = (self.gt, self.n_gt) if pairs is None else (ops.CSR(pairs[0], pairs[1]), int(pairs[2]))
        return ops.rank_positions(kind, users_tab, user_ids, items_tab, csr, sig_u, sig_i, c, self.mask, n_pairs=n_pairs)

    @staticmethod
    def _branch_factors(kind, users_tab, user_ids, branch_tab, w, wu):
        """(sig_u, sig_i) of a position count: sigmoid(e_u . w_user) of the queries, sigmoid(row . w) of branch_tab's rows"""
        sig_u = sig_i = None
        both = kind in (ops.SCORE_RUBI_BOTH, ops.SCORE_DIRECT_MINUS_BOTH)
        if both and branch_tab.shape[1] == users_tab.shape[1]:
            sig_i, sig_u = ops.branch_sigmoid2(branch_tab, w, None, users_tab, wu, user_ids)
        elif kind != ops.SCORE_NORMAL:
            sig_i = ops.branch_sigmoid(branch_tab, w)
            if both:
                sig_u = ops.branch_sigmoid(users_tab, wu, user_ids)
        return sig_u, sig_i

    def rank_report(self, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None, group_of=None, n_groups=None):
        """rank_report.summarize of rank_positions: {'users', 'pairs', 'skipped', 'auc', 'mrr', 'mpr'} and, with group_of
        (n_items group ids), 'group_pairs' / 'group_mpr' -- AUC, reciprocal rank and rank percentile of the held-out
        items over the whole catalogue, not the first K.  One device-to-host copy (the positions)."""
        pos = self.rank_positions(kind, users_tab, user_ids, items_tab, w, wu, c, branch)
        return self._summarize_positions(pos, group_of, n_groups)

    # ------------------------------------------------------------------ the same over item shards (MACR_SHARD_RANK_REPORT=1)
    def _rank_shard(self, kind, users_tab, user_ids, items_tab, w, wu, branch, whole_factors=None):
        """This rank's shard for a position count, resolved as rank_local resolves it -- a replicated table cut by
        item_shard_range, local_items_range, the strided set_local_items -- as the arguments of ops.rank_shard_*:
        (rows of the shard or None when it is empty, sig_u, sig_i, item_lo, item_stride); the branch factors are those of
        the shard's rows (branch: sharded like items_tab).  whole_factors: (sig_u, sig_i) of a replicated table's rows,
        already computed -- the shard takes its slice instead of launching them again."""
        lo, hi, rows = self._shard(items_tab)
        if self._local_own is not None:
            lo, stride = self._local_own.lo, self._local_own.stride
        else:
            if self.local_items_range is None and items_tab.shape[0] != self.n_items:
                raise _lib.MacrError(_lib.E_INVALID, "rank_positions_sharded: %d item rows for an evaluator of %d items"
                                     % (items_tab.shape[0], self.n_items))
            stride = 1
        if rows.shape[0] == 0:
            return None, None, None, lo, stride
        if whole_factors is not None:
            sig_u, sig_i = whole_factors[0], None if whole_factors[1] is None else whole_factors[1][lo:hi]
        else:
            sig_u, sig_i = self._branch_factors(kind, users_tab, user_ids, rows if branch is None else self._shard(branch)[2], w, wu)
        return rows, sig_u, sig_i, lo, stride

    def rank_shard_keys(self, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None, shard=None):
        """First phase of rank_positions_sharded on this rank's shard: int64[n_gt], the (score, GLOBAL id) key of every
        held-out pair whose item the shard holds, 0 elsewhere (ops.rank_shard_keys); the sum over the ranks is complete.
        shard: what _rank_shard returned for these arguments, where the caller has it (one set of branch factors for
        both phases)."""
        rows, sig_u, sig_i, lo, stride = shard or self._rank_shard(kind, users_tab, user_ids, items_tab, w, wu, branch)
        if rows is None:
            return torch.zeros(self.n_gt, dtype=torch.int64, device=self.device)
        return ops.rank_shard_keys(kind, users_tab, user_ids, rows, self.gt, sig_u, sig_i, c, lo, stride, n_pairs=self.n_gt)

    def rank_shard_counts(self, keys, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None, shard=None):
        """Second phase: int64[n_gt], this shard's share of every pair's position given the complete keys -- its items
        before the key, minus those of them the query's train list (the GLOBAL mask) holds, flagged where the shard holds
        the pair's item and the train list holds it too (ops.rank_shard_counts).  shard: as in rank_shard_keys."""
        rows, sig_u, sig_i, lo, stride = shard or self._rank_shard(kind, users_tab, user_ids, items_tab, w, wu, branch)
        if rows is None:
            return torch.zeros(self.n_gt, dtype=torch.int64, device=self.device)
        return ops.rank_shard_counts(kind, users_tab, user_ids, rows, self.gt, keys, sig_u, sig_i, c, self.mask, lo, stride,
                                     n_pairs=self.n_gt)

    def rank_positions_sharded(self, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None):
        """rank_positions for any item sharding: int32[n_gt] on the device, the same on every rank and equal to what
        rank_positions returns from one rank on the whole table.  Every rank calls it (two all-reduces of 8 bytes per pair:
        the keys, the counts); in a world of one rank with the whole table it is rank_positions by other kernels.  A
        position is a count over the catalogue and the shards partition it: the shards' integer counts against one
        (score, global id) key add up, in any order.  A replicated table needs no key exchange: model.sync() and
        broadcast_params have made the replicas equal, so every rank scores the pairs on the whole table itself.  The
        branch factors are launched once and serve both phases."""
        if self.n_gt == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        args = (kind, users_tab, user_ids, items_tab, w, wu, c, branch)
        if self._local_own is None and self.local_items_range is None:
            whole = self._branch_factors(kind, users_tab, user_ids, items_tab if branch is None else branch, w, wu)
            shard = self._rank_shard(kind, users_tab, user_ids, items_tab, w, wu, branch, whole_factors=whole)
            keys = ops.rank_shard_keys(kind, users_tab, user_ids, items_tab, self.gt, whole[0], whole[1], c, 0, 1, n_pairs=self.n_gt)
        else:
            shard = self._rank_shard(kind, users_tab, user_ids, items_tab, w, wu, branch)
            keys = sharding.sum_over_ranks(self.rank_shard_keys(*args, shard=shard))
        counts = sharding.sum_over_ranks(self.rank_shard_counts(keys, *args, shard=shard))
        return ops.rank_shard_combine(keys, counts)

    def rank_report_sharded(self, kind, users_tab, user_ids, items_tab, w=None, wu=None, c=0.0, branch=None, group_of=None,
                            n_groups=None):
        """rank_report with rank_positions_sharded underneath: the same dict on every rank, for any item sharding"""
        pos = self.rank_positions_sharded(kind, users_tab, user_ids, items_tab, w, wu, c, branch)
        return self._summarize_positions(pos, group_of, n_groups)

    def _summarize_positions(self, pos, group_of, n_groups):
        from . import rank_report
        pos = pos.cpu().numpy()
        if getattr(self, "_gt_host", None) is None:
            mask_len = np.array([len(set(row)) for row in self._mask_lists], dtype=np.int64)
            self._gt_host = (self.gt.ptr.cpu().numpy(), self.gt.idx[:self.n_gt].cpu().numpy(), self.n_items - mask_len)
        gt_ptr, gt_idx, n_cand = self._gt_host
        if group_of is not None:
            group_of = np.asarray(group_of.cpu() if torch.is_tensor(group_of) else group_of)
        return rank_report.summarize(pos, gt_ptr, gt_idx, n_cand, group_of, n_groups)

    # ------------------------------------------------------------------ MF flavour
    def test_mf(self, kind, users_tab, user_ids, items_tab, Ks, w=None, wu=None, c=0.0, branch=None):
        """-> {'precision','recall','ndcg','hit_ratio'}: np.ndarray(len(Ks)) float64, the mean over the
        query users (train.py:286-290 accumulates re[...]/n_test_users)."""
        m = self._means("mf", kind, users_tab, user_ids, items_tab, tuple(Ks), w, wu, c, branch).cpu().numpy()
        return {'precision': m[0].copy(), 'recall': m[1].copy(), 'ndcg': m[2].copy(), 'hit_ratio': m[3].copy()}

    def _finish(self, flavour, vals, idx, Ks, out=None):
        """(W,U,K) lists (splits of one shard, or the gathered shards) -> column means of the per-user metrics.
        out: optional pinned host tensor the last kernel writes the means to."""
        if flavour == "mf":
            if vals.shape[0] == 1:
                ix, cnt = idx[0], None    # one sorted list per query: nothing to merge (the metrics kernel counts a list's ids itself)
            else:
                _, ix, cnt = ops.topk_merge(vals, idx)
            if not self.fold_metrics:
                return ops.colmean(ops.metrics_mf(ix, cnt, self.gt, list(Ks)), out=out)         # (U,4,nK) float64 -> (4,nK)
            # metrics and their means over the queries in one launch (macr_metrics_mf_mean); its scratch is this evaluator's
            # own (a captured graph bakes the address in)
            if len(Ks) not in self._mean_ws:
                self._mean_ws[len(Ks)] = ops.metrics_mf_mean_workspace(idx.shape[1], len(Ks), idx.device)
            return ops.metrics_mf_mean(ix, cnt, self.gt, list(Ks), self._mean_ws[len(Ks)], out=out)   # (4,nK) float64
        if vals.shape[0] == 1 and vals.shape[2] <= _lib.MAX_TOPK and self._local_own is None:
            # one sorted list per query: the metrics kernel completes short lists with the masked ids itself (-inf fill,
            # batch_test.py:124-134) -- no merge launch
            return ops.colmean(ops.metrics_foldout(idx[0], self.gt, hr_in_ap_slot=True, fill_mask=self.mask), out=out)
        _, ix, _ = ops.topk_merge(vals, idx, self.mask)                                      # -inf fill, batch_test.py:124-134
        return ops.colmean(ops.metrics_foldout(ix, self.gt, hr_in_ap_slot=True), out=out)   # (U,5*max_top) fp32

    def _direct(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch=None, **launch):
        vals, idx = self.rank_local(kind, users_tab, user_ids, items_tab, max(Ks), w, wu, c, branch, **launch)
        if sharding.world()[1] > 1:
            lv, li, _ = ops.topk_merge(vals, idx)
            vals, idx = sharding.gather_topk(lv, li)
        return self._finish(flavour, vals, idx, Ks)

    def _c_scalar(self, c):
        """The evaluator's device copy of c: kernels read it at run time (macr_score_topk c_dev), so the captured
        graph of an evaluation serves every c of a sweep -- only this scalar is rewritten between replays."""
        if self._c_host != float(c):
            self._c_dev.fill_(float(c))
            self._c_host = float(c)
        return self._c_dev

    def _means(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch=None):
        """The device part of an evaluation.  An evaluator ranks the same queries against the same (in-place updated)
        tables every epoch, and the ~14 launches of one evaluation are issued from Python between two host
        synchronisations: on one GPU the sequence is captured once into a HIP graph and replayed (one launch instead
        of ~90 us of launch gaps per evaluation).  c is not part of the sequence: the kernels read it from a device
        scalar at run time, so the c sweep of the tuners (tune.py:545-578) replays ONE graph.  Anything else that changes
        the sequence -- other tensors, K -- is another graph; `use_graph = False` launches directly.  With several ranks
        the sequence is two graphs around the one collective (all-gather of the shards' top-K)."""
        c = self._c_scalar(c)
        world = sharding.world()[1]
        if (self.optimistic and self.use_graph and world == 1 and self.device.type == "cuda"
                and self.n_queries <= self.max_queries_per_pass and max(Ks) <= _lib.MAX_TOPK_FUSED):
            return self._means_optimistic(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch)
        self._last_info = None
        # (no seeds yet for this K and shard: the first ranking samples, and leaves them -- the warm-up run of a capture
        # creates the seeds: the capture itself must not pick them up)
        seeded = self._seed_feedback() and self.n_queries <= self.max_queries_per_pass and self._has_seeds(max(Ks), items_tab.shape[0], branch)
        try:
            return self._means_launch(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, world, branch,
                                      seeded=seeded, filter=self.filter_now)[0]
        finally:
            self._stats_readback(seeded)

    def _means_optimistic(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch=None):
        """First round only, results in pinned host memory; the rest of the ranking when the first round says so."""
        self._stats_evt = None                    # (a stats copy of the complete path still in flight: not needed any more)
        seeded, self._policy = eval_policy.seed_first_round(self._policy, self.use_seeds,
                                                            self._has_seeds(max(Ks), items_tab.shape[0], branch))
        used = self.filter_now

        def launch(mode, repair_of=None):
            return self._means_launch(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, 1, branch,
                                      seeded=seeded, mode=mode, repair_of=repair_of, filter=used)
        out, entry, ran_complete = launch("first")
        torch.cuda.current_stream().synchronize()
        self._last_seeded = False                 # (nothing for _seed_feedback to read later)
        relisted, fallback = self._stats_first.tolist()[0], 0
        redone = relisted != 0
        if ran_complete:
            # graph replay was just switched off and the COMPLETE sequence ran in place of the first round: what it relisted and
            # whether it fell back are in its own statistics (the bf16 back-off must see a fallback there too)
            relisted, fallback = self._stats.tolist()
        elif not redone:
            self.fast_stats["fast"] += 1
        else:
            # a list overflowed or seeds were stale: the repair round (and, behind it, the exact fallback) on the first round's
            # workspace and outputs -- what the complete call would have launched
            self.fast_stats["redone"] += 1
            out = launch("repair", entry[3])[0]
            torch.cuda.current_stream().synchronize()
            fallback = int(self._stats_first[1])
        self._last_info = {"seeded": seeded, "query_blocks_relisted": relisted, "exact_fallback": fallback, "redone": redone,
                           "filter": used}
        self._policy = eval_policy.after_outcome(self._policy, self.filter, used, seeded, relisted, fallback, redone,
                                                 eval_policy.relist_tolerance(self.n_queries), ran_complete)
        return out.clone()

    def last_eval_info(self):
        """What the last evaluation did: {"seeded": its thresholds came from the previous ranking's candidates,
        "query_blocks_relisted": blocks of 256 queries whose lists overflowed / whose seeds were stale, "exact_fallback",
        "redone": the first round did not stand and the complete sequence ran (optimistic mode)}.  Synchronises."""
        if self._last_info is not None:
            return dict(self._last_info)
        st = self._stats.tolist()
        return {"seeded": bool(self._last_seeded), "query_blocks_relisted": st[0], "exact_fallback": st[1], "redone": False}

    # ------------------------------------------------------------------ graph cache
    def _captured(self, key, shape_key, direct, capture, scratch):
        """A launch sequence the cache has no graph of: warm-up run, capture, keep-alive list -> the new entry
        (stages, out, keep, first_bufs), or None where graph replay has just been switched off (shape_key given: misses count).
        capture() -> (stages, out, first_bufs); scratch(): the cached buffers the launches touched."""
        if shape_key is not None:
            # capturing costs about two evaluations: callers that keep changing the sequence are better off launching directly
            # Misses are counted per evaluation SHAPE (tables, query set, score kind, Ks, stream): one shape legitimately needs up
            # to 8 graphs (first / repair round x candidate filter x seeded or not), so a run that evaluates two query sets and
            # meets a back-off must not lose graph replay.  A caller whose tensors change from call to call shows up as many
            # shapes, or as one shape asking for more graphs than its key space has.
            misses = self._graph_misses_by_shape
            misses[shape_key] = misses.get(shape_key, 0) + 1
            self._graph_misses += 1
            if misses[shape_key] > 8 or len(misses) > 8:
                self.use_graph = False
                self._graphs.clear()
                return None
        direct()                                  # warm-up: allocations, caches, attributes
        torch.cuda.synchronize()
        stages, out, first_bufs = capture()
        # the graphs bake in the addresses of everything they touched: keep the inputs and the cached scratch
        # (ranking workspace, mask bitmaps) alive for as long as they exist, whatever the caches do later
        entry = self._graphs[key] = (stages, out, scratch(), first_bufs)
        return entry

    @staticmethod
    def _replay(entry):
        (ga, local, gathered, gb), out = entry[0], entry[1]
        ga.replay()
        if gb is not None:
            nv, ni = sharding.gather_topk(local[0], local[1])
            gathered[0].copy_(nv); gathered[1].copy_(ni)
            gb.replay()
        return out

    def _means_launch(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, world, branch=None, repair_of=None, **launch):
        """-> (means, graph entry or None, the complete sequence ran in place of the first round asked for).
        launch: what rank_local is told (seeded, mode, filter) -- and, with the tensors, the graph's key."""
        tensors = (users_tab, user_ids, items_tab, w, wu, c, branch)
        direct = lambda **kw: self._direct(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch, **kw)
        if not self.use_graph:
            return direct(repair_of=repair_of, **launch), None, False
        mode = launch.get("mode")
        host_out = None
        if mode:
            hk = (flavour, Ks)
            if hk not in self._host_out:
                shape = (4, len(Ks)) if flavour == "mf" else (5 * max(Ks),)
                self._host_out[hk] = torch.zeros(shape, dtype=torch.float64).pin_memory()
            host_out = self._host_out[hk]
        shape_key = (flavour, kind, Ks, torch.cuda.current_stream().cuda_stream, world) + _ptrs(users_tab, user_ids, items_tab, w, wu, branch)
        key = shape_key + tuple(sorted(launch.items()))
        entry = self._graphs.get(key)
        if entry is None:
            K = max(Ks)

            def capture():
                if world == 1:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        vals, idx = self.rank_local(kind, users_tab, user_ids, items_tab, K, w, wu, c, branch, repair_of=repair_of, **launch)
                        out = self._finish(flavour, vals, idx, Ks, out=host_out)
                    # what a repair round must continue on: the first round's outputs AND the workspace it was captured with
                    # (the per-device cache is regrown whenever a larger evaluator asks: ops._topk_workspace)
                    return (g, None, None, None), out, (vals, idx, ops._topk_ws_cache.get(items_tab.device))
                # several ranks: the collective stays outside -- one graph up to this shard's merged lists, the
                # all-gather (RCCL), one graph from the gathered lists to the means
                ga = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga):
                    vals, idx = self.rank_local(kind, users_tab, user_ids, items_tab, K, w, wu, c, branch, **launch)
                    lv, li, _ = ops.topk_merge(vals, idx)
                gv, gi = sharding.gather_topk(lv, li)                    # static inputs of the second graph
                gb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gb):
                    out = self._finish(flavour, gv, gi, Ks)
                return (ga, (lv, li), (gv, gi), gb), out, None

            def scratch():
                keep = list(tensors) + [ops._topk_ws_cache.get(items_tab.device)] + list(self._seeds.values())
                local = [] if self._local_own is None else [self._mask_local] + list(self._mask_local.__dict__.get("_row_ranges", {}).values())
                for csr in [self.mask] + list(self.mask.__dict__.get("_row_ranges", {}).values()) + local:
                    keep.extend(csr.__dict__.get("_mask_bits", {}).values())
                return keep
            entry = self._captured(key, shape_key, lambda: direct(repair_of=repair_of, **launch), capture, scratch)
            if entry is None:                     # graph replay switched off
                if mode != "first":
                    return direct(repair_of=repair_of, **launch), None, False
                # the complete sequence: its result needs no check, and its own statistics are in self._stats
                self._stats_first.zero_()
                return direct(**dict(launch, mode=None)), None, True
        return self._replay(entry), entry, False

    # ------------------------------------------------------------------ c sweep (tuners)
    def _sweep_direct(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c_dev, branch=None):
        sig_i = ops.branch_sigmoid(items_tab if branch is None else branch, w)
        sig_u = ops.branch_sigmoid(users_tab, wu, user_ids) if kind in (ops.SCORE_RUBI_BOTH, ops.SCORE_DIRECT_MINUS_BOTH) else None
        vals, idx = ops.score_topk_sweep(kind, users_tab, user_ids, items_tab, max(Ks), sig_u, sig_i, c_dev, self.mask, 0,
                                         filter=self.filter)
        return torch.stack([self._finish(flavour, vals[g:g + 1], idx[g:g + 1], Ks) for g in range(c_dev.numel())])

    def sweep_means(self, flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, cs, branch=None):
        """Column means of the per-user metrics for every c of `cs`, (len(cs), ...).  On one GPU the values go through
        the shared-listing-pass kernel in groups of up to four (one captured graph per group size, the group's values
        in a device array the kernels read at run time); item-sharded runs evaluate c by c."""
        cs = [float(c) for c in cs]
        # The shared-listing-pass kernels follow the candidate filter (k_score_stream_bs under "bf16": 0.31 ms per value
        # on the Gowalla shape against 0.43 one evaluation at a time, tools/bench_sweep.py).  MACR_SWEEP_ONE_BY_ONE=1
        # sends every value through the seeded, graph-replayed single evaluation instead (A/B switch).
        one_by_one = os.environ.get("MACR_SWEEP_ONE_BY_ONE", "0") == "1"
        if (one_by_one or sharding.world()[1] > 1 or kind == ops.SCORE_NORMAL or self.n_queries > self.max_queries_per_pass
                or max(Ks) > _lib.MAX_TOPK_FUSED):           # (the shared-listing-pass kernels rank K <= 32)
            return torch.stack([self._means(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c, branch).clone() for c in cs])
        outs = []
        for a in range(0, len(cs), _lib.MAX_SWEEP):
            chunk = cs[a:a + _lib.MAX_SWEEP]
            n = len(chunk)
            if n not in self._c_sweep:
                self._c_sweep[n] = torch.zeros(n, dtype=torch.float32, device=self.device)
            c_dev = self._c_sweep[n]
            c_dev.copy_(torch.tensor(chunk, dtype=torch.float32), non_blocking=False)
            direct = lambda: self._sweep_direct(flavour, kind, users_tab, user_ids, items_tab, Ks, w, wu, c_dev, branch)
            if not self.use_graph:
                outs.append(direct().clone())
                continue
            key = ("sweep", n, flavour, self.filter, kind, Ks, torch.cuda.current_stream().cuda_stream) + _ptrs(users_tab, user_ids, items_tab, w, wu, branch)
            entry = self._graphs.get(key)
            if entry is None:
                def capture():
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        out = direct()
                    return (g, None, None, None), out, None
                scratch = lambda: ([users_tab, user_ids, items_tab, w, wu, c_dev, branch, ops._sweep_ws_cache.get(items_tab.device)]
                                   + list(self.mask.__dict__.get("_mask_bits", {}).values()))
                entry = self._captured(key, None, direct, capture, scratch)       # (a sweep's graphs are no misses)
            outs.append(self._replay(entry).clone())
        return torch.cat(outs)

    def test_mf_sweep(self, kind, users_tab, user_ids, items_tab, Ks, w, wu, cs, branch=None):
        """test_mf for every c of `cs` -> list of result dicts (the c sweep of macr_mf/tune.py:545-578)."""
        m = self.sweep_means("mf", kind, users_tab, user_ids, items_tab, tuple(Ks), w, wu, cs, branch).cpu().numpy()
        return [{'precision': x[0].copy(), 'recall': x[1].copy(), 'ndcg': x[2].copy(), 'hit_ratio': x[3].copy()} for x in m]

    def test_lgcn_sweep(self, kind, users_tab, user_ids, items_tab, Ks, w, wu, cs, branch=None):
        top_show = np.sort(np.asarray(Ks))
        max_top = int(top_show.max())
        m = self.sweep_means("lgcn", kind, users_tab, user_ids, items_tab, tuple(Ks), w, wu, cs, branch).cpu().numpy()
        out = []
        for x in m:
            final = x.reshape(5, max_top)[:, top_show - 1]
            out.append({'hr': final[2].copy(), 'recall': final[1].copy(), 'ndcg': final[3].copy()})
        return out

    # ------------------------------------------------------------------ LightGCN flavour
    def test_lgcn(self, kind, users_tab, user_ids, items_tab, Ks, w=None, wu=None, c=0.0, branch=None):
        """-> {'hr','recall','ndcg'}: np.ndarray(len(Ks)) (batch_test.py:134-161): C++-style fp32 prefix
        metrics, HR := 1[recall@k != 0], mean over users, columns Ks-1 in ascending-K order."""
        top_show = np.sort(np.asarray(Ks))
        max_top = int(top_show.max())
        final = self._means("lgcn", kind, users_tab, user_ids, items_tab, tuple(Ks), w, wu, c, branch).cpu().numpy()
        final = final.reshape(5, max_top)[:, top_show - 1]
        return {'hr': final[2].copy(), 'recall': final[1].copy(), 'ndcg': final[3].copy()}


def _policy_field(name):
    """`_seed_skip` ... `_bf16_backoff`: the policy's counters, readable and writable (bench.py resets `_seed_skip`)"""
    return property(lambda self: getattr(self._policy, name),
                    lambda self, value: setattr(self, "_policy", self._policy._replace(**{name: value})))


for _name in eval_policy.State._fields:
    setattr(Evaluator, "_" + _name, _policy_field(_name))


def eval_score_matrix_foldout(score_matrix, test_items, top_k=20, thread_num=None):
    """Drop-in for macr_lightgcn/evaluator/cpp/evaluate_foldout.py:12-18 backed by the HIP kernels
    (macr_topk_scores + macr_metrics_foldout).  score_matrix: (U,N) array-like with train items already
    at -inf (batch_test.py:129); test_items: list of per-user ground-truth id lists.
    Returns np.float32 (U, 5*top_k) laid out [precision|recall|ap|ndcg|mrr].  thread_num is accepted and
    ignored.  Ties rank by ascending item id (the C++ leaves tie order to std::partial_sort_copy)."""
    if len(score_matrix) != len(test_items):
        raise ValueError("The lengths of score_matrix and test_items are not equal.")
    dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(score_matrix, torch.Tensor):
        scores = score_matrix.to(device=dev, dtype=torch.float32).contiguous()
    else:
        scores = torch.from_numpy(np.ascontiguousarray(score_matrix, dtype=np.float32)).to(dev)
    idx, _ = ops.topk_scores(scores, top_k, want_vals=False)
    gt = ops.CSR.from_lists(test_items, dev)
    return ops.metrics_foldout(idx, gt).cpu().numpy()
