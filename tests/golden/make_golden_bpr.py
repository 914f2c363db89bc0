#!/usr/bin/env python3
"""G11: golden losses / gradients of the two BPR losses, computed by the reference's own graph code.

    macr_mf/model.py           BPRMF.create_bpr_loss (:264-275)           -- `--train normal`, trained by `opt` (:52-57)
    macr_lightgcn/LightGCN.py  LightGCN.create_bpr_loss (:398-413)        -- `--loss bpr` (the parser's default), `opt` (:173-178)

executed exactly as tests/golden/make_golden_model.py executes the other loss builders (its functional `tensorflow`
stand-in and its runners are imported, not copied), on the SAME problems as G10: MF cases a / b / c, LightGCN cases a / b
(same seeds and shapes, so the inputs are G10's arrays; this script checks that).  Each case runs in float32 and float64.
Only outputs are stored (tests/golden/G11_bpr_steps.npz): losses of both runs, gradients of the float64 run (the float32
gradients agree with them to ~1e-6 relative on these cases).  No reference text travels.

Usage:  python tests/golden/make_golden_bpr.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as G  # noqa: E402

# the problems of make_golden_model.main (seed, n_users, n_items, d, B, scale | n_inter) and its hyper-parameters
MF_CASES = {"a": (11, 60, 40, 32, 48, 0.3), "b": (12, 300, 80, 64, 257, 0.6), "c": (13, 90, 50, 32, 96, 1.5)}
LGCN_CASES = {"a": (31, 70, 45, 32, 64, 400), "b": (32, 260, 150, 64, 200, 1500)}
HYPER = dict(alpha=1e-2, beta=1e-3, decay=1e-5, batch_size=1024)


def load_builders():
    G.install()
    sys.path.insert(0, os.path.join(G.REF, "macr_mf"))
    sys.argv = ["make_golden_bpr"]
    BPRMF = importlib.import_module("model").BPRMF
    # LightGCN.py without its import-time harness (as make_golden_model.main does it)
    sys.path.insert(0, os.path.join(G.REF, "macr_lightgcn"))
    helper = types.ModuleType("utility.helper")
    bt = types.ModuleType("utility.batch_test")
    bt.args = types.SimpleNamespace(gpu_id=0)
    helper.np = bt.np = np
    sys.modules.update({"utility": types.ModuleType("utility"), "utility.helper": helper, "utility.batch_test": bt})
    return BPRMF, importlib.import_module("LightGCN").LightGCN


def main():
    BPRMF, LightGCN = load_builders()
    g10 = {}
    for f in sorted(os.listdir(HERE)):
        if f.startswith("G10_model_steps_") and f.endswith(".npz"):
            with np.load(os.path.join(HERE, f)) as z:
                g10.update((k, z[k]) for k in z.files)
    out = {}
    for tag, (seed, nu, ni, d, B, scale) in MF_CASES.items():
        prob = G.mf_problem(seed, nu, ni, d, B, scale)
        for k, v in zip(("P", "Q", "w", "wu", "u", "i", "j"), prob):
            assert np.array_equal(v, g10["mf_%s/%s" % (tag, k)]), (tag, k)
        for dt, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
            res = G.run_mf_loss(BPRMF, "create_bpr_loss", prob, HYPER, dt)
            for k, v in res.items():
                if dname == "f64" or np.ndim(v) == 0:
                    out["mf_%s/bpr/%s/%s" % (tag, dname, k)] = np.asarray(v)
    for tag, (seed, nu, ni, d, B, n_inter) in LGCN_CASES.items():
        prob = G.lgcn_problem(seed, nu, ni, d, B, n_inter)
        for k, v in zip(("P", "Q", "w", "wu", "u", "i", "j"), prob[1:]):
            assert np.array_equal(v, g10["lgcn_%s/%s" % (tag, k)]), (tag, k)
        assert np.array_equal(prob[0].data, g10["lgcn_%s/data" % tag])
        for dt, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
            res = G.run_lgcn(LightGCN, "create_bpr_loss", prob, HYPER, 2, dt)
            for k, v in res.items():
                if k in ("ua", "ia"):
                    continue                                  # the propagation is G10's
                if dname == "f64" or np.ndim(v) == 0:
                    out["lgcn_%s/bpr/%s/%s" % (tag, dname, k)] = np.asarray(v)
    out["hyper"] = np.asarray([HYPER["alpha"], HYPER["beta"], HYPER["decay"], HYPER["batch_size"]], np.float64)
    path = os.path.join(HERE, "G11_bpr_steps.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KB)" % (path, len(out), os.path.getsize(path) / 1024))
    for tag in MF_CASES:
        print("mf_%s    loss f32 %.6f f64 %.6f" % (tag, out["mf_%s/bpr/f32/loss" % tag], out["mf_%s/bpr/f64/loss" % tag]))
    for tag in LGCN_CASES:
        print("lgcn_%s  loss f32 %.6f f64 %.6f" % (tag, out["lgcn_%s/bpr/f32/loss" % tag], out["lgcn_%s/bpr/f64/loss" % tag]))


if __name__ == "__main__":
    main()
