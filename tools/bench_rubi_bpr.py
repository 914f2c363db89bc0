#!/usr/bin/env python3
"""Per-step and per-kernel time of the MF two-branch BPR loss (--train rubi, MACR_LOSS_RUBIBPR) against --train rubibce
(MACR_LOSS_RUBIBCE) -- the same step around a different (B,B) cell -- at the Gowalla shape (29 858 x 40 981, d = 64,
B = 4096) and the ML-10M shape (B = 8192).
    step     deferred steps as bench.py times them: regions of 20 steps, the flush inside the region, synchronize on both
             sides, the median region reported; the two kinds alternate region by region in one process
    kernels  macr_timing_begin / macr_timing_end (a HIP event after every launch of the library) over deferred steps
             (`bxb+adam`: the (B,B) launch with the riding Adam blocks) and over complete steps (`bxb`: the (B,B) launch alone)
Usage: python tools/bench_rubi_bpr.py [--steps 20] [--regions 60] [--out profiles/mf_rubi_bpr.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from macr_amd import ops, synth  # noqa: E402

KINDS = {"rubibce": ops.LOSS_RUBIBCE, "rubi": ops.LOSS_RUBIBPR}


def run_steps(state, kind, batches, n, defer):
    for k in range(n):
        b = batches[k % batches.shape[0]]
        state.step(kind, b[0], b[1], b[2], defer=defer)
    state.flush()


def timed_region(state, kind, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run_steps(state, kind, batches, n, True)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / n


def kernel_times(state, kind, batches, n, defer):
    """{kernel name: mean microseconds per launch} over n steps (the flush's launches included under their own names).  The
    library keeps at most 256 marks per timing_begin: n steps of at most 6 launches each must stay below that."""
    assert 6 * n + 2 < 256, n
    ops.timing_begin()
    run_steps(state, kind, batches, n, defer)
    marks = ops.timing_end(256)
    assert len(marks) < 256, "timing marks overflowed: %d launches" % len(marks)
    sums, counts = {}, {}
    for name, ms in marks:
        sums[name] = sums.get(name, 0.0) + 1e3 * ms
        counts[name] = counts.get(name, 0) + 1
    return {k: round(sums[k] / counts[k], 3) for k in sums}


def shape(name, B, a, dev):
    cfg = synth.WORKLOADS[name]
    n_u, n_i, d = cfg["n_users"], cfg["n_items"], 64
    gen = torch.Generator(device=dev).manual_seed(1)
    P, Q = synth.xavier_table(n_u, d, gen, dev), synth.xavier_table(n_i, d, gen, dev)
    w = synth.xavier_table(d, 1, gen, dev).reshape(-1)
    hyper = ops.make_hyper(cfg["lr"], cfg["regs"], cfg["alpha"], cfg["beta"], B)
    states = {k: ops.MFState(P.clone(), Q.clone(), w.clone(), w.clone(), hyper, B) for k in KINDS}
    batches = synth.train_batches(64, n_u, n_i, B, gen, dev)
    for k, kind in KINDS.items():                          # warm-up: workspaces, first touch, clocks
        run_steps(states[k], kind, batches, 40, True)
    us = {k: [] for k in KINDS}
    for _ in range(a.regions):
        for k, kind in KINDS.items():
            us[k].append(timed_region(states[k], kind, batches, a.steps))
    out = {"n_users": n_u, "n_items": n_i, "d": d, "B": B}
    med = {k: float(np.median(v)) for k, v in us.items()}
    out["step_us"] = {k: {"median": round(med[k], 2), "min": round(min(us[k]), 2), "max": round(max(us[k]), 2)} for k in KINDS}
    out["step_rubi_over_rubibce"] = round(med["rubi"] / med["rubibce"], 4)
    deferred, complete = {}, {}
    for rep in range(3):                                   # alternate here too; keep the last (warm) repetition
        for k, kind in KINDS.items():
            deferred[k] = kernel_times(states[k], kind, batches, 32, True)
            complete[k] = kernel_times(states[k], kind, batches, 32, False)
    out["kernels_deferred_us"], out["kernels_complete_us"] = deferred, complete
    out["bxb_adam_rubi_over_rubibce"] = round(deferred["rubi"]["bxb+adam"] / deferred["rubibce"]["bxb+adam"], 4)
    out["bxb_rubi_over_rubibce"] = round(complete["rubi"]["bxb"] / complete["rubibce"]["bxb"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mf_rubi_bpr.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"steps_per_region": a.steps, "regions": a.regions, "device": torch.cuda.get_device_name(0),
           "gowalla_B4096": shape("gowalla", 4096, a, dev), "ml10m_B8192": shape("ml10m", 8192, a, dev)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
