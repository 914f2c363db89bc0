"""The (B,B) loss kernel's choice between its arithmetic forms (k_bxb, macr_amd/csrc/train_kernels.hip) at the edges of its
window, against the oracle (-m gpu).  A wave takes the fast form iff every column of its tile has p amax >= -20 and
YLO <= n bmax <= 6 (YLO = -60 with rows in pairs, R = 2 / 4; -20 with R = 1) and amax, bmax <= 1; full batches take up to 8
flagged columns of a tile (p < -20, n > 6, n < -60) out of the rotation into the launch's neutral blocks.  The batches of
tests/bxb_cases.py sit 0.5 % inside and outside each of those comparisons, with exactly 8 and 9 flags in a tile, 8 flags inside
one lane of the neutral block's scan, a tile flagged by column yet fast by its wave's test, and rows with a == 1.0f;
tests/test_bxb_cases_cpu.py shows without a GPU that every such wave is really there and that the oracle itself is within a
third of the tolerances below of the float64 graph.  Per case (bxb_cases.run_on_gpu): one complete step -- losses 1e-5,
first-step gradients of P, Q, w, wu at rtol 5e-4 / atol 2e-6 max, everything finite, scratch zero -- and a twin that takes
the batch twice deferred (the kernel's instantiation with the pending dense Adam pass), both losses 1e-5.

A case that fails: bxb_cases.classify says which form each wave took; the exact form is the reference's arithmetic, so a
failure that stays with the offending tile exact by its inputs points at the neutral bookkeeping (slab ncb of the row sums, the
-2 per evaluation taken back out of the log sum, which launch part owns a column's colpart)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bxb_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    assert not [k for k in os.environ if k.startswith("MACR_BXB_")], "the in-process cases are laid out for the default launch"
    from macr_amd import ops as _ops
    return _ops


def _record(record_property, name, res):
    cls = bc.oracle_forward(bc.case(name))["cls"]
    record_property(name + "_labels", bc.label_counts(cls))
    for k in ("loss_rel", "deferred_rel", "grad_P", "grad_Q", "grad_w", "grad_wu"):
        record_property("%s_%s" % (name, k), res[k])


@pytest.mark.parametrize("name", bc.IN_PROCESS)
def test_form_edges_follow_the_oracle(ops, name, record_property):
    """partial_r1 (B = 300) and partial_r4 (B = 4100, pad rows in the last row group of 256): fast and exact waves on either
    side of p amax = -20, n bmax = 6 and n bmax = YLO, an edge column in the partial tile; full_r1 (B = 1280) and full_r4
    (B = 4096): the neutral route with tiles of 8 flags (in one lane of the scan, spread over its four lanes, beyond column
    1024) and of 9 (all inside the wave's window: fast; one outside: exact); item_branch_a1 (rubibce, B = 512): rows with
    sig(si) == 1.0f, raw p = -19.9 fast at amax == 1 and p = -20.1 neutralised."""
    c = bc.case(name)
    assert c["R"] == bc.default_rows(c["B"]) and not c["env"]
    _record(record_property, name, bc.run_on_gpu(ops, name))


@pytest.fixture(scope="module")
def default_losses(ops):
    """neutral_off's batch under the default launch (neutral blocks on), in this process"""
    return bc.run_on_gpu(ops, "neutral_on")["losses"]


_child_failed = []


@pytest.mark.parametrize("setting", sorted(bc.WORKER_SETTINGS))
def test_form_edges_under_the_launch_knobs(ops, setting, default_losses, record_property):
    """MACR_BXB_ROWS = 2 and = 4 (B = 300 and 512: the partial and the full layout with YLO = -60, rows in pairs; R = 2 runs
    nowhere else) and MACR_BXB_NEUTRAL = 0 (B = 512: the full layout with every flagged tile left to its exact waves, losses
    also within 2e-6 of the default launch's -- two routes of the same arithmetic, the bound of
    test_mf_deferred_adam_equals_complete_steps).  One child process per setting (tests/bxb_knob_worker.py), one at a time;
    after a child that failed or ran out of time no further child is started."""
    if _child_failed:
        pytest.fail("not started: the child for %s failed" % _child_failed[0])
    torch.cuda.synchronize()
    env = {k: v for k, v in os.environ.items() if not k.startswith("MACR_BXB_")}
    env.update(bc.CASES[bc.WORKER_SETTINGS[setting][0]]["env"])
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "bxb_knob_worker.py"), setting], env=env, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    except subprocess.TimeoutExpired:
        _child_failed.append(setting)
        raise
    if r.returncode != 0:
        _child_failed.append(setting)
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ok"] and verdict["setting"] == setting, verdict
    assert sorted(verdict["cases"]) == sorted(bc.WORKER_SETTINGS[setting])
    for name, res in verdict["cases"].items():
        _record(record_property, name, res)
    if setting == "neutral0":
        got = np.asarray(verdict["cases"]["neutral_off"]["losses"], np.float32)
        want = np.asarray(default_losses, np.float32)
        rel = float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
        record_property("neutral_off_vs_default_rel", rel)
        print("neutral_off: losses %r, default launch %r, max rel %.3e" % (got.tolist(), want.tolist(), rel))
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)
