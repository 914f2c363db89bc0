#!/usr/bin/env python3
"""What the rank-count-invariant row-sharded MF step (HipBackend(invariant=True), MACR_SHARD_INVARIANT=1) costs: per-step time of
the default, the deterministic and the invariant sharded step on the same shards and batches, the three alternating region by
region in one process, at a world of ONE rank (the replicated step: gather, forward, (B,B), backward, apply; the collectives
of the split step are not in these numbers -- its extra wire bytes are computed below, not measured).
    shapes   gowalla  29 858 x 40 981,      d = 64,  B = 4096, rubibceboth, the dense Adam pass every step (K = 1)
             large    1 000 000 x 100 000,  d = 128, B = 8192, rubibceboth, the lazy pass with the period the shard size gives
                      (sharded_train.lazy_period_for: K > 1)
    step     RowShardedMF.step; regions of --steps steps, the flush inside the region, a device synchronise on both sides, the
             MEDIAN of --regions (>= 50) regions reported with their minimum and maximum
    kernels  macr_timing_begin / macr_timing_end (a HIP event after every launch of the library): mean microseconds per launch
             and kernel name, over the steps of a region of each mode
No bound is set on the cost: it is measured and written down.
Usage: python tools/bench_shard_invariant.py [--steps 20] [--regions 60] [--out profiles/shard_invariant.txt]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, sharded_train, synth  # noqa: E402

# name, n_users, n_items, d, B, lazy period (None: by shard size)
CASES = (("gowalla", 29858, 40981, 64, 4096, 1), ("large", 1000000, 100000, 128, 8192, None))
MODES = ("default", "deterministic", "invariant")


def run_steps(model, batches, n):
    for k in range(n):
        b = batches[k % batches.shape[0]]
        model.step(b[0], b[1], b[2])
    model.flush()


def timed_region(model, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(model, batches, n)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def kernel_times(model, batches, n):
    """[(kernel name, mean microseconds per launch, launches per step)] over n steps, in launch order"""
    ops.timing_begin()
    run_steps(model, batches, n)
    marks = ops.timing_end(256)
    assert len(marks) < 256, "timing marks overflowed: %d launches" % len(marks)
    order, sums, counts = [], {}, {}
    for name, ms in marks:
        if name not in sums:
            order.append(name)
        sums[name] = sums.get(name, 0.0) + 1e3 * ms
        counts[name] = counts.get(name, 0) + 1
    return [(k, sums[k] / counts[k], counts[k] / float(n)) for k in order]


def case(name, n_u, n_i, d, B, lazy, a, dev, say):
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    hyper = ops.make_hyper(1e-3, 1e-5, 1e-3, 1e-3, B)
    models = {}
    for m in MODES:
        backend = sharded_train.HipBackend(ops.LOSS_RUBIBCEBOTH, d, hyper, dev, deterministic=(m == "deterministic"),
                                           invariant=(m == "invariant"))
        models[m] = sharded_train.RowShardedMF(None, None, w, w, backend, rank=0, world=1,
                                               shards=(P.clone(), Q.clone(), n_u, n_i), lazy_period=lazy)
    K = models["default"].lazy_period
    assert all(models[m].lazy_period == K for m in MODES)
    assert models["deterministic"].deterministic and not models["default"].deterministic and not models["default"].invariant
    assert models["invariant"].invariant and not models["invariant"].deterministic
    batches = synth.train_batches(64, n_u, n_i, B, gen, dev)          # (Zipf positives: hot rows)
    for m in MODES:                                        # warm-up: workspaces, first touch, clocks, every sweep phase of the lazy pass
        run_steps(models[m], batches, max(40, 2 * K))
    us = {m: [] for m in MODES}
    for _ in range(a.regions):
        for m in MODES:
            us[m].append(timed_region(models[m], batches, a.steps))
    med = {m: float(np.median(us[m])) for m in MODES}
    say("%s %d x %d, d = %d, B = %d, rubibceboth, world 1, %s" % (name, n_u, n_i, d, B,
                                                                 "dense Adam pass" if K == 1 else "lazy Adam pass, K = %d" % K))
    for m in MODES:
        say("  %-13s step %8.2f us  median of %d regions of %d steps  [min %.2f, max %.2f]" % (m, med[m], a.regions, a.steps,
                                                                                             min(us[m]), max(us[m])))
    say("  deterministic / default = %.3f   invariant / default = %.3f   invariant / deterministic = %.3f" % (
        med["deterministic"] / med["default"], med["invariant"] / med["default"], med["invariant"] / med["deterministic"]))
    for m in MODES:
        for rep in range(2):                               # keep the second (warm) repetition
            rows = kernel_times(models[m], batches, 8)
        say("  %-13s kernels of a step: %s" % (m, ", ".join("%s %.1f us%s" % (k, t, "" if c == 1 else " x%g" % c) for k, t, c in rows)))
    # the split step's branch all-reduce at W > 1: the complete block-row region instead of the 8 folded rows (computed)
    blocks = -(-B // (1024 // d))
    say("  split form, branch all-reduce per rank and step: %d block rows x 2 d floats = %d bytes (default: 8 rows = %d bytes; "
        "deterministic: W x %d bytes); forward region: unchanged (deterministic: W x its bytes)" % (
            blocks, blocks * 2 * d * 4, 8 * 2 * d * 4, 8 * 2 * d * 4))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shard_invariant.txt"))
    a = ap.parse_args()
    assert a.regions >= 50, "medians of at least 50 regions"
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_shard_invariant.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("Row-sharded MF training step: default, deterministic, invariant (tools/bench_shard_invariant.py --steps %d --regions %d) on %s" % (
        a.steps, a.regions, torch.cuda.get_device_name(0)))
    for name, n_u, n_i, d, B, lazy in CASES:
        case(name, n_u, n_i, d, B, lazy, a, dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
