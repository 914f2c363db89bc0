"""The arms of the native code that only an environment switch selects, each in a fresh child process (-m gpu).

MACR_STAGE_LISTED, MACR_STAGING, MACR_EVAL_F32_SAMPLE and MACR_LGCN_DENSE are latched by a `static const` the first time a
process consults them, so every setting runs tests/switch_worker.py in a child of its own: the arm against the CPU oracle
(or the float64 restatements of the BPR kinds), with the launch names that prove the arm ran.  INTEGRATION.md B.4 promises
that none of these switches changes a result beyond the order of floating-point additions; the tolerances are those of the
tests that hold the default arms to the same references.

    stage_listed0   MACR_STAGE_LISTED=0: B = 20000, gradient rows staged in batch order and found through the sorted list
                    (seg_sum and the indexed Adam pass with the list's values); one child per (d, batch flavour) -- the CPU
                    oracle of one rubibceboth step at B = 20000 takes ~3 s, so a child is three of those, not twelve
    staging1        MACR_STAGING=1: the staged path below 8193 triples (a batch smaller than one sort tile), all five MF loss
                    kinds and one LightGCN shape
    f32_sample      MACR_EVAL_F32_SAMPLE=f32: the fp32 sampling pass under the fp32 filter; f32_sample_off: the sibling
                    without the variable, where the same call samples on the fp16 copies
    lgcn_dense      MACR_LGCN_DENSE=1: the environment's form of MACR_STEP_DENSE_LAYERS

One child at a time; this process launches nothing while one runs; after a child that failed or ran out of time no further
child is started."""
import json
import os
import subprocess
import sys

import pytest
import torch

import switch_worker as sw

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

CHILDREN = [("stage_listed0", part) for part in sw.STAGE_LISTED_PARTS] + [("staging1", None), ("f32_sample", None),
                                                                          ("f32_sample_off", None), ("lgcn_dense", None)]
_child_failed = []


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def run_child(setting, part):
    if _child_failed:
        pytest.fail("not started: the child for %s failed" % _child_failed[0])
    torch.cuda.synchronize()
    env = {k: v for k, v in os.environ.items() if not k.startswith("MACR_")}
    env.update(sw.ENV[setting])
    name = setting if part is None else "%s %s" % (setting, part)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "switch_worker.py"), setting] + ([] if part is None else [part]),
                           env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    except subprocess.TimeoutExpired:
        _child_failed.append(name)
        raise
    if r.returncode != 0:
        _child_failed.append(name)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0, (r.returncode, lines[-1][-6000:] if lines else "", r.stderr[-4000:])
    verdict = json.loads(lines[-1])
    print(json.dumps({k: verdict[k] for k in ("setting", "part", "env", "names", "losses")}))
    assert verdict["ok"] and verdict["setting"] == setting and verdict["part"] == part and verdict["env"] == sw.ENV[setting], verdict
    return verdict


def all_names(verdict):
    out = set()
    for v in verdict["names"].values():
        for names in (v.values() if isinstance(v, dict) else [v]):
            out.update(names)
    return out


@pytest.mark.parametrize("setting,part", CHILDREN, ids=["-".join(x for x in c if x) for c in CHILDREN])
def test_switch_arm_in_a_fresh_process(ops, setting, part):
    verdict = run_child(setting, part)
    names = all_names(verdict)
    # (the worker asserts the names call by call; this is the same statement about the verdict a reader sees)
    if setting == "stage_listed0":
        assert {"ref_sort", "seg_index", "seg_sum", "adam_indexed"} <= names and "ref_place" not in names, names
        assert len(verdict["names"]) == 6                                # two loss kinds, three steps each
    elif setting == "staging1":
        assert "ref_sort" in names and "batch_sort" not in names, names
        assert len(verdict["losses"]) == len(sw.STAGING_SHAPES) * 5 + 2
    elif setting == "f32_sample":
        assert "score_sample" in names and "score_sample_b" not in names and "tau_seed" in names, names
        assert len(verdict["names"]) == 5 * 4 * 2                       # every score kind, d and K
    elif setting == "f32_sample_off":
        assert all("score_sample_b" in v["unseeded"] and "score_sample" not in v["unseeded"] for v in verdict["names"].values()), verdict["names"]
    elif setting == "lgcn_dense":
        assert "adam_dense" in names and "lgcn_finalize" not in names, names
