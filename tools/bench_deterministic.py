#!/usr/bin/env python3
"""What the bit-reproducible MF step (MFState(deterministic=True), MACR_STEP_DETERMINISTIC) costs: per-step time of the default
and of the deterministic step on the same tables and batches, the two alternating region by region in one process.
    shapes   addressa  13 485 x 744,     d = 64, B = 1024,  rubibceboth
             gowalla   29 858 x 40 981,  d = 64, B = 4096,  rubibceboth and normalbce
             gowalla   29 858 x 40 981,  d = 64, B = 65536, normalbce
    step     as the training loop runs it: deferred steps for rubibceboth, complete steps for normalbce; regions of
             --steps steps, the flush inside the region, a device synchronise on both sides, the MEDIAN of --regions (>= 50)
             regions reported with their minimum and maximum
    kernels  macr_timing_begin / macr_timing_end (a HIP event after every launch of the library): mean microseconds per launch
             and kernel name, over complete steps of each mode
No bound is set on the cost: it is measured and written down.
Usage: python tools/bench_deterministic.py [--steps 20] [--regions 60] [--out profiles/deterministic.txt]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402

CASES = (("addressa", 1024, "rubibceboth"), ("gowalla", 4096, "rubibceboth"), ("gowalla", 4096, "normalbce"),
         ("gowalla", 65536, "normalbce"))
KIND = {"rubibceboth": ops.LOSS_RUBIBCEBOTH, "normalbce": ops.LOSS_NORMALBCE}
MODES = ("default", "deterministic")


def run_steps(state, kind, batches, n, defer):
    for k in range(n):
        b = batches[k % batches.shape[0]]
        state.step(kind, b[0], b[1], b[2], defer=defer)
    state.flush()


def timed_region(state, kind, batches, n, defer):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(state, kind, batches, n, defer)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def kernel_times(state, kind, batches, n):
    """[(kernel name, mean microseconds per launch, launches per step)] over n complete steps, in launch order"""
    ops.timing_begin()
    run_steps(state, kind, batches, n, False)
    marks = ops.timing_end(256)
    assert len(marks) < 256, "timing marks overflowed: %d launches" % len(marks)
    order, sums, counts = [], {}, {}
    for name, ms in marks:
        if name not in sums:
            order.append(name)
        sums[name] = sums.get(name, 0.0) + 1e3 * ms
        counts[name] = counts.get(name, 0) + 1
    return [(k, sums[k] / counts[k], counts[k] / float(n)) for k in order]


def case(name, B, train, a, dev, say):
    cfg = synth.WORKLOADS[name]
    n_u, n_i, d = cfg["n_users"], cfg["n_items"], 64
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    hyper = ops.make_hyper(cfg["lr"], cfg["regs"], cfg["alpha"], cfg["beta"], B)
    states = {m: ops.MFState(P.clone(), Q.clone(), w.clone(), w.clone(), hyper, B, deterministic=(m == "deterministic")) for m in MODES}
    batches = synth.train_batches(16 if B > 8192 else 64, n_u, n_i, B, gen, dev)          # (Zipf positives: hot rows)
    kind, defer = KIND[train], train == "rubibceboth"
    for m in MODES:                                        # warm-up: workspaces, first touch, clocks
        run_steps(states[m], kind, batches, 40, defer)
    us = {m: [] for m in MODES}
    for _ in range(a.regions):
        for m in MODES:
            us[m].append(timed_region(states[m], kind, batches, a.steps, defer))
    med = {m: float(np.median(us[m])) for m in MODES}
    say("%s %d x %d, d = %d, B = %d, %s (%s steps)" % (name, n_u, n_i, d, B, train, "deferred" if defer else "complete"))
    for m in MODES:
        say("  %-13s step %8.2f us  median of %d regions of %d steps  [min %.2f, max %.2f]" % (m, med[m], a.regions, a.steps,
                                                                                             min(us[m]), max(us[m])))
    say("  deterministic / default = %.3f" % (med["deterministic"] / med["default"]))
    for m in MODES:
        for rep in range(2):                               # keep the second (warm) repetition
            rows = kernel_times(states[m], kind, batches, 8)
        say("  %-13s kernels of a complete step: %s" % (m, ", ".join("%s %.1f us%s" % (k, t, "" if c == 1 else " x%g" % c) for k, t, c in rows)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deterministic.txt"))
    a = ap.parse_args()
    assert a.regions >= 50, "medians of at least 50 regions"
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_deterministic.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("MF training step, default against deterministic (tools/bench_deterministic.py --steps %d --regions %d) on %s" % (
        a.steps, a.regions, torch.cuda.get_device_name(0)))
    for name, B, train in CASES:
        case(name, B, train, a, dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
