#!/usr/bin/env python3
"""G13: golden losses / gradients of the MF two-branch BPR loss (`--train rubi`), computed by the reference's own graph code.

    macr_mf/model.py  BPRMF.create_bpr_loss_two_brach (:124-156)  -- trained by `opt_two` (:64-66)

executed exactly as tests/golden/make_golden_model.py executes the other loss builders (its functional `tensorflow`
stand-in and `run_mf_loss` are imported, not copied), on G10's MF problems a / b / c (same seeds and shapes, so the inputs
are G10's arrays; this script checks that) and on case d = mf_problem(14, 90, 50, 32, 96, 1.7), whose (B,B) logits reach
[-71.7, 57.7]: every cell is finite in float32 although two of them together overflow a shared logarithm.  Each case runs
in float32 and float64.  Only outputs are stored (tests/golden/G13_mf_rubi_bpr.npz): losses of both runs, dP / dQ / dw of the
float64 run -- and the inputs of case d, which G10 does not hold.  The float64 run's dwu is checked to be zero here (the
loss has no user branch).  No reference text travels.

Usage:  python tests/golden/make_golden_rubi_bpr.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as G  # noqa: E402

MF_CASES = {"a": (11, 60, 40, 32, 48, 0.3), "b": (12, 300, 80, 64, 257, 0.6), "c": (13, 90, 50, 32, 96, 1.5),
            "d": (14, 90, 50, 32, 96, 1.7)}
HYPER = dict(alpha=1e-2, beta=1e-3, decay=1e-5, batch_size=1024)
INPUTS = ("P", "Q", "w", "wu", "u", "i", "j")


def main():
    G.install()
    sys.path.insert(0, os.path.join(G.REF, "macr_mf"))
    sys.argv = ["make_golden_rubi_bpr"]
    BPRMF = importlib.import_module("model").BPRMF
    g10 = {}
    for f in sorted(os.listdir(HERE)):
        if f.startswith("G10_model_steps_") and f.endswith(".npz"):
            with np.load(os.path.join(HERE, f)) as z:
                g10.update((k, z[k]) for k in z.files)
    out = {}
    for tag, (seed, nu, ni, d, B, scale) in MF_CASES.items():
        prob = G.mf_problem(seed, nu, ni, d, B, scale)
        for k, v in zip(INPUTS, prob):
            if tag == "d":
                out["mf_d/in/%s" % k] = v
            else:
                assert np.array_equal(v, g10["mf_%s/%s" % (tag, k)]), (tag, k)
        for dt, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
            res = G.run_mf_loss(BPRMF, "create_bpr_loss_two_brach", prob, HYPER, dt)
            assert np.isfinite(res["loss"]), (tag, dname)
            assert not res["dwu"].any(), (tag, dname)                     # no user branch: w_user has no gradient
            for k in ("loss", "mf_loss", "reg_loss"):
                out["mf_%s/rubi_bpr/%s/%s" % (tag, dname, k)] = np.asarray(res[k])
            if dname == "f64":
                for k in ("dP", "dQ", "dw"):
                    out["mf_%s/rubi_bpr/f64/%s" % (tag, k)] = np.asarray(res[k])
    out["hyper"] = np.asarray([HYPER["alpha"], HYPER["beta"], HYPER["decay"], HYPER["batch_size"]], np.float64)
    path = os.path.join(HERE, "G13_mf_rubi_bpr.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KB)" % (path, len(out), os.path.getsize(path) / 1024))
    for tag in MF_CASES:
        print("mf_%s    loss f32 %.6f f64 %.6f" % (tag, out["mf_%s/rubi_bpr/f32/loss" % tag], out["mf_%s/rubi_bpr/f64/loss" % tag]))


if __name__ == "__main__":
    main()
