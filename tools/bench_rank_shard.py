#!/usr/bin/env python3
"""Time of the item-sharded position count (macr_rank_shard_keys + macr_rank_shard_counts + macr_rank_shard_combine) beside the
unsharded call (macr_rank_positions), in the method of tools/bench_rank_positions.py: the library's own per-kernel timing
(macr_timing_*: a hipEvent after every launch), warmed up, median of the repeats, each call in a timing window of its own,
the two sequences ALTERNATING in one process.

Shape: the Gowalla evaluation shape of tools/bench_rank_positions.py -- 15 424 query users x 40 981 items, d = 64, the tables
of an MF model trained for a few epochs, rubi_both at c = 40, 13 held-out items per user (200 512 pairs).

  world 1      the whole table as one shard (item_lo 0, stride 1): keys + counts + combine against macr_rank_positions,
               held to 1.10 x the unsharded call (the same counting and mask subtraction plus two short launches)
  one of 8     the interleaved shard of rank 0 of 8 (rows 0, 8, 16, ...: 5 123 of them): its keys and its counts beside an
               eighth of the unsharded counting pass -- whether the pass scales with the shard; no bound
  existing     --unsharded-only times macr_rank_positions alone and prints one JSON line: it uses nothing the parent commit
               lacks, so a copy of this file runs inside a checkout of the parent; run the two builds alternately in one
               GPU session, collect the lines in a file and pass it with --runs: the report records both sets and says
               whether they overlap
The collectives (two int64 all-reduces of 8 bytes x pairs) are not timed: one card has no xGMI to time them on.

Usage: python tools/bench_rank_shard.py [--repeats 50] [--epochs 3] [--unsharded-only --label NAME] [--runs FILE] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_rank_positions as brp  # noqa: E402
from macr_amd import ops, synth  # noqa: E402
from macr_amd.evaluator import Evaluator  # noqa: E402

KIND, C = brp.KIND, brp.C
SHARD_KERNELS = ("rank_shard_keys", "rank_shard_reset", "rank_shard_cols", "rank_shard_count", "rank_shard_finish",
                 "rank_shard_combine")
WORLD = 8


def alternating(calls, repeats, warmup=10):
    """{name: {kernel: median microseconds}} of several calls taken in turn, each in a timing window of its own"""
    seen = {name: {} for name in calls}
    for r in range(warmup + repeats):
        for name, call in calls.items():
            ops.timing_begin()
            call()
            for kernel, ms in ops.timing_end():
                if r >= warmup:
                    seen[name].setdefault(kernel, []).append(1e3 * ms)
    return {name: {k: float(np.median(v)) for k, v in per.items()} for name, per in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--unsharded-only", action="store_true", help="time macr_rank_positions alone and print one JSON line")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--runs", default=None, help="file of --unsharded-only lines of this build and the parent's, taken alternately")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, state = brp.model(dev, a.epochs)
    users, mask, gt = synth.eval_problem(cfg, seed=3)
    uid = torch.from_numpy(users).to(dev)
    n_i, d = cfg["n_items"], cfg["d"]
    ev = Evaluator(mask, gt, n_i, dev)
    pairs, n_pairs = ev.gt, ev.n_gt
    sig_i, sig_u = ops.branch_sigmoid2(state.Q, state.w, None, state.P, state.wu, uid)
    whole = lambda: ops.rank_positions(KIND, state.P, uid, state.Q, pairs, sig_u, sig_i, C, ev.mask, n_pairs=n_pairs)
    if a.unsharded_only:
        med = alternating({"whole": whole}, a.repeats)["whole"]
        print(json.dumps({"lib": a.label, "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
                          "total": round(sum(med[k] for k in brp.RANK_KERNELS), 2), **{k: round(med[k], 2) for k in brp.RANK_KERNELS}}))
        return

    def world1():
        keys = ops.rank_shard_keys(KIND, state.P, uid, state.Q, pairs, sig_u, sig_i, C, 0, 1, n_pairs=n_pairs)
        counts = ops.rank_shard_counts(KIND, state.P, uid, state.Q, pairs, keys, sig_u, sig_i, C, ev.mask, 0, 1, n_pairs=n_pairs)
        return ops.rank_shard_combine(keys, counts)
    want = whole()
    assert torch.equal(world1(), want), "world 1: the sharded sequence and macr_rank_positions disagree"
    # the eight interleaved shards once, for the answer; rank 0's under the timer
    shards = [(state.Q[r::WORLD].contiguous(), sig_i[r::WORLD].contiguous(), r) for r in range(WORLD)]
    keys = sum(ops.rank_shard_keys(KIND, state.P, uid, q, pairs, sig_u, s, C, r, WORLD, n_pairs=n_pairs) for q, s, r in shards)
    counts = sum(ops.rank_shard_counts(KIND, state.P, uid, q, pairs, keys, sig_u, s, C, ev.mask, r, WORLD, n_pairs=n_pairs)
                 for q, s, r in shards)
    assert torch.equal(ops.rank_shard_combine(keys, counts), want), "8 interleaved shards and macr_rank_positions disagree"
    q0, s0, _ = shards[0]

    def one_of_8():
        ops.rank_shard_keys(KIND, state.P, uid, q0, pairs, sig_u, s0, C, 0, WORLD, n_pairs=n_pairs)
        ops.rank_shard_counts(KIND, state.P, uid, q0, pairs, keys, sig_u, s0, C, ev.mask, 0, WORLD, n_pairs=n_pairs)
    med = alternating({"whole": whole, "world1": world1, "one_of_8": one_of_8}, a.repeats)
    tot = lambda per, names: sum(per.get(k, 0.0) for k in names)
    t_whole, t_w1 = tot(med["whole"], brp.RANK_KERNELS), tot(med["world1"], SHARD_KERNELS)
    t_8 = tot(med["one_of_8"], SHARD_KERNELS)
    fmt = lambda per, names: " + ".join("%s %.1f" % (k, per[k]) for k in names if k in per)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "users": len(users), "n_items": n_i, "d": d,
           "pairs": n_pairs, "whole": {k: round(v, 2) for k, v in med["whole"].items()}, "whole_total": round(t_whole, 2),
           "world1": {k: round(v, 2) for k, v in med["world1"].items()}, "world1_total": round(t_w1, 2),
           "world1_ratio": round(t_w1 / t_whole, 4), "world1_within_1_10": bool(t_w1 <= 1.10 * t_whole),
           "one_of_8_rows": int(q0.shape[0]), "one_of_8": {k: round(v, 2) for k, v in med["one_of_8"].items()},
           "one_of_8_total": round(t_8, 2), "eighth_of_rank_count": round(med["whole"]["rank_count"] / WORLD, 2),
           "collective_bytes_per_rank": 2 * 8 * n_pairs}
    lines = ["%s, median of %d, microseconds, the calls alternating; %d users x %d items, d = %d, %d pairs; positions equal in "
             "all three forms" % (res["device"], a.repeats, len(users), n_i, d, n_pairs),
             "unsharded   macr_rank_positions: %s = %.1f" % (fmt(med["whole"], brp.RANK_KERNELS), t_whole),
             "world 1     keys + counts + combine on the whole table: %s = %.1f: %.3f x the unsharded call, bound 1.10 x (%s)" % (
                 fmt(med["world1"], SHARD_KERNELS), t_w1, t_w1 / t_whole, "met" if res["world1_within_1_10"] else "MISSED"),
             "one of 8    interleaved shard of %d rows, keys + counts: %s = %.1f; its counting pass %.1f beside an eighth of the "
             "unsharded counting pass %.1f" % (q0.shape[0], fmt(med["one_of_8"], SHARD_KERNELS), t_8,
                                               med["one_of_8"]["rank_shard_count"], res["eighth_of_rank_count"]),
             "collectives per rank at W > 1: 2 x 8 bytes x %d pairs = %d bytes (computed, not measured: one card)" % (
                 n_pairs, res["collective_bytes_per_rank"])]
    if a.runs:
        runs = [json.loads(l) for l in open(a.runs) if l.strip().startswith("{")]
        by = {}
        for r in runs:
            by.setdefault(r["lib"], []).append(r["total"])
            lines.append("existing    macr_rank_positions, %s: %s = %.1f" % (r["lib"], fmt(r, brp.RANK_KERNELS), r["total"]))
        res["existing_path"] = by
        if len(by) == 2:
            (la, va), (lb, vb) = by.items()
            overlap = max(min(va), min(vb)) <= min(max(va), max(vb))
            res["existing_path_overlap"] = bool(overlap)
            lines.append("existing    %s %s, %s %s: the two sets %s" % (la, va, lb, vb, "overlap" if overlap else "DO NOT overlap"))
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
