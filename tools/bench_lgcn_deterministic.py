#!/usr/bin/env python3
"""What the bit-reproducible LightGCN step (LGCNState(deterministic=True), MACR_STEP_DETERMINISTIC) costs: per-step time of the
default and of the deterministic step on the same graph, table and batches, the two alternating region by region in one process.
    shapes   yelp2018  31 668 x 38 048, d = 64, 2 layers, B = 4096, bceboth  (the graph, table and batches of
                       bench.py --workload yelp2018)
             addressa  13 485 x 744,    d = 64, 2 layers, B = 1024, bceboth  (the shape of the README's Addressa LightGCN command)
    step     complete steps as the training loop runs them; regions of --steps steps, a device synchronise on both sides, the
             MEDIAN of --regions (>= 50) regions reported with their minimum and maximum
    kernels  macr_timing_begin / macr_timing_end (a HIP event after every launch of the library): per launch of ONE complete
             step, in launch order, the median microseconds over --kernel-steps steps of each mode
No bound is set on the cost: it is measured and written down.
Usage: python tools/bench_lgcn_deterministic.py [--steps 20] [--regions 60] [--out profiles/lgcn_deterministic.txt]"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402

CASES = (("yelp2018", {}), ("addressa", dict(alpha=1e-2)))       # (the LightGCN command's --alpha; synth's is the MF command's)
MODES = ("default", "deterministic")
KIND, LAYERS = ops.LOSS_RUBIBCEBOTH, 2


def run_steps(state, batches, n, first=0):
    for k in range(n):
        b = batches[(first + k) % batches.shape[0]]
        state.step(KIND, b[0], b[1], b[2])


def timed_region(state, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(state, batches, n)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def kernel_times(state, batches, n):
    """[(kernel name, median microseconds)] per launch of one complete step, in launch order, over n steps"""
    per_step = []
    for k in range(n):
        ops.timing_begin()
        run_steps(state, batches, 1, first=k)
        marks = ops.timing_end(256)
        assert len(marks) < 256, "timing marks overflowed: %d launches" % len(marks)
        per_step.append(marks)
    names = [name for name, _ in per_step[0]]
    assert all([name for name, _ in m] == names for m in per_step), "the steps of one mode launch the same kernels"
    return [(name, float(np.median([1e3 * m[k][1] for m in per_step]))) for k, name in enumerate(names)]


def case(name, override, a, dev, say):
    cfg = dict(synth.WORKLOADS[name], **override)
    n_u, n_i, d, B = cfg["n_users"], cfg["n_items"], cfg["d"], cfg["batch"]
    _, A = synth.lgcn_graph(cfg, seed=9)
    gen = torch.Generator(device=dev).manual_seed(12345)
    T = synth.xavier_table(n_u + n_i, d, gen, dev)
    w, wu = synth.xavier_table(d, 1, gen, dev).reshape(-1), synth.xavier_table(d, 1, gen, dev).reshape(-1)
    adj = ops.CSR.from_scipy(A, dev)
    hyper = ops.make_hyper(cfg["lr"], cfg["regs"], cfg["alpha"], cfg["beta"], B)
    states = {m: ops.LGCNState(T.clone(), n_u, n_i, w.clone(), wu.clone(), adj, LAYERS, hyper, B, deterministic=(m == "deterministic"))
              for m in MODES}
    batches = synth.train_batches(64, n_u, n_i, B, gen, dev)          # (Zipf positives: hot rows)
    for m in MODES:                                        # warm-up: workspaces, first touch, clocks
        run_steps(states[m], batches, 40)
    us = {m: [] for m in MODES}
    for _ in range(a.regions):
        for m in MODES:
            us[m].append(timed_region(states[m], batches, a.steps))
    med = {m: float(np.median(us[m])) for m in MODES}
    say("%s %d x %d (nnz %d), d = %d, %d layers, B = %d, bceboth" % (name, n_u, n_i, A.nnz, d, LAYERS, B))
    for m in MODES:
        say("  %-13s step %8.2f us  median of %d regions of %d steps  [min %.2f, max %.2f]" % (m, med[m], a.regions, a.steps,
                                                                                             min(us[m]), max(us[m])))
    say("  deterministic / default = %.3f" % (med["deterministic"] / med["default"]))
    for m in MODES:
        rows = kernel_times(states[m], batches, a.kernel_steps)
        say("  %-13s kernels of one complete step (sum %.1f us): %s" % (m, sum(t for _, t in rows),
                                                                      ", ".join("%s %.1f" % (k, t) for k, t in rows)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--kernel-steps", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lgcn_deterministic.txt"))
    a = ap.parse_args()
    assert a.regions >= 50, "medians of at least 50 regions"
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_lgcn_deterministic.py needs an MI355X: nothing is timed without one")
    dev = torch.device("cuda")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("LightGCN training step, default against deterministic (tools/bench_lgcn_deterministic.py --steps %d --regions %d) on %s" % (
        a.steps, a.regions, torch.cuda.get_device_name(0)))
    for name, override in CASES:
        case(name, override, a, dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
