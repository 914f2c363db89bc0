"""The evaluator's seeding and candidate-filter policy: integer bookkeeping, no device, no native library.

Every choice here only moves time around: whichever filter ranks and wherever its thresholds come from, the ranking is the
fp32 ranking bit for bit.  The state is immutable; the evaluator replaces it (`self._policy = ...`), so a copy of an
evaluator never shares counters with it.
"""
from typing import NamedTuple

LP_FILTERS = ("bf16", "f16")        # reduced-precision candidate filters (fp32 re-scoring; include/macr_hip.h MACR_EVAL_FILTER_*)
MAX_BACKOFF = 16


class State(NamedTuple):
    # seeding policy: thresholds come from the previous ranking unless that went badly last time
    seed_skip: int = 0
    seed_backoff: int = 1
    # ... and one tier above the bf16 filter: the fp16 filter's margin is 12x the bf16 filter's.  An UNSEEDED fp16 evaluation that
    # had to list query blocks again (lists that overflowed under a threshold less that margin: scores at the top closer
    # together than fp16 resolves, e.g. (y - c) sig_i sig_u with c = 30 on barely trained rows of d = 128), or one that
    # ended in the exact kernel, sends the next 1, 2, 4 ... 16 evaluations to the bf16 filter (whose own back-off leads on to fp32).
    f16_skip: int = 0
    f16_backoff: int = 1
    # filter policy (the same shape): a bf16-filter evaluation that ended in the exact kernel -- candidate lists overflowed in
    # both rounds: scores packed tighter at the top than the filter's error bound resolves, e.g. a catalogue of a million
    # barely trained items under c = 40 -- cost 2-3x an fp32-filter evaluation; the next 1, 2, 4 ... 16 evaluations take the
    # fp32 filter before bf16 is tried again.  The ranking is the same either way.
    bf16_skip: int = 0
    bf16_backoff: int = 1


def _tier(skip, backoff, failed, redone):
    """(skip, back-off) of a tier after an evaluation that tried it.  failed: the next `backoff` evaluations go without it
    and the back-off doubles (1, 2, 4 ... 16); it stood: back-off 1 again; an evaluation that was redone for another
    reason leaves the back-off where it is"""
    if failed:
        return backoff, min(MAX_BACKOFF, 2 * backoff)
    return skip, (backoff if redone else 1)


def filter_now(configured, s):
    """the candidate filter of the ranking about to be launched: `configured`, or the tier below it ("bf16", then "f32")
    while a reduced-precision filter is backed off"""
    if configured == "f16" and s.f16_skip == 0:
        return "f16"
    if configured in LP_FILTERS:
        return "f32" if s.bf16_skip > 0 else "bf16"
    return configured


def relist_tolerance(n_queries):
    """blocks of 256 queries a seeded ranking may list twice before the seeds count as stale: none up to 63 blocks (a repair
    round costs what an unseeded ranking costs there), one per 64 blocks beyond -- on 100 000 queries a handful of
    re-listed blocks is a few queries with degenerate scores (every item tied), not a model that moved away from its seeds,
    and the sampling pass would cost every block more than their repair does"""
    return ((n_queries + 255) // 256) // 64


def seeds_allowed(use_seeds, world):
    """Several ranks: no seeds.  The policy's state is per shard, so ranks would switch between the seeded and the
    sampled launch sequence -- and capture the other graph, with its extra warm-up collectives -- at different
    evaluations: mismatched all-gathers.  (A 1/8 shard's sampling pass is 13 us; there is little to win.)"""
    return use_seeds and world == 1


def seed_first_round(s, use_seeds, has_seeds):
    """First-round path, before the ranking: -> (it takes its thresholds from the seeds, state).  An evaluation of a
    back-off is spent whether or not there were seeds to skip; what the ranking found follows in after_outcome."""
    seeded = bool(use_seeds and s.seed_skip == 0 and has_seeds)
    if use_seeds and s.seed_skip > 0:
        s = s._replace(seed_skip=s.seed_skip - 1)
    return seeded, s


def seed_complete(s, use_seeds, world, relisted, tolerance):
    """Complete path: decide, before a ranking is launched, whether it takes its thresholds from the seeds (if it has any)
    -> (seeded, state).  relisted: of the previous SEEDED ranking, whose stats have arrived since (None: nothing pending) --
    whether blocks of 256 queries had to be listed twice because a seeded threshold was too loose (macr_score_topk stats).
    The repair round costs about as much as an unseeded ranking however few blocks it lists, so one of them means the
    model still moves too far between two evaluations for seeds to pay (early epochs): the next 1, 2, 4 ... 16 evaluations
    use the sampling pass before seeds are tried again."""
    if not seeds_allowed(use_seeds, world):
        return False, s
    skip, backoff = s.seed_skip, s.seed_backoff
    if relisted is not None:
        skip, backoff = _tier(skip, backoff, relisted > tolerance, False)
    return skip == 0, s._replace(seed_skip=max(0, skip - 1), seed_backoff=backoff)


def after_outcome(s, configured, used, seeded, relisted, exact_fallback, redone, tolerance, ran_complete=False):
    """First-round path, after the evaluation: the state once it is known what the ranking under filter `used` found.
    relisted: query blocks listed twice; redone: the first round did not stand; ran_complete: graph replay was switched
    off under this evaluation and the complete sequence ran in place of the first round -- that tells the filter tiers
    what they need and the seeds nothing.  (The complete path never comes here: it leaves the filter tiers alone.)
    `redone` with neither trigger leaves a back-off where it is."""
    seed_skip, seed_backoff, f16_skip, f16_backoff, bf16_skip, bf16_backoff = s
    if seeded and not ran_complete:
        seed_skip, seed_backoff = _tier(seed_skip, seed_backoff, relisted > tolerance, redone)
    if used == "f16":
        f16_skip, f16_backoff = _tier(f16_skip, f16_backoff, exact_fallback or (not seeded and relisted), redone)
    else:
        if configured == "f16" and f16_skip > 0 and not (used == "f32" and bf16_skip > 0):
            f16_skip -= 1                # (an evaluation spent in the bf16 tier; fp32 ones count for the bf16 tier's own wait)
        if used == "bf16":
            bf16_skip, bf16_backoff = _tier(bf16_skip, bf16_backoff, exact_fallback, redone)
        elif bf16_skip > 0:
            bf16_skip -= 1
    return State(seed_skip, seed_backoff, f16_skip, f16_backoff, bf16_skip, bf16_backoff)
