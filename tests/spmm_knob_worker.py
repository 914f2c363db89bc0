"""Worker of tests/test_gpu_spmm_hubs.py::test_launch_switches_in_a_fresh_process: the launch-side SpMM switches
(MACR_SPMM_STREAM_FUSED, MACR_SPMM_RECORDS, MACR_LGCN_BWD1_DENSE) are latched by the first launch of a process, so each
setting gets a process of its own with the switches in its environment.  Runs the exact SMALL d = 64 propagation and one
training case of tests/spmm_cases.py, checks the kernel names the setting must select, prints a JSON verdict.

    python tests/spmm_knob_worker.py stream_fused | records0 | bwd1_sparse | bwd1_dense
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import spmm_cases as sc  # noqa: E402


def main(setting):
    from macr_amd import ops
    env = {k: os.environ[k] for k in sc.PLAN_KNOBS if k in os.environ}       # the plan-time part of this process's setting
    res = {"setting": setting, "env": {k: v for k, v in os.environ.items() if k.startswith(("MACR_SPMM_", "MACR_LGCN_"))}}
    # test a's SMALL d = 64 case under this process's switches
    names = []
    for L in (1, 2):
        case = sc.exact_case(sc.small(), 64, L)
        adj = sc.device_csr(ops, case["A"], env)
        names += sc.run_exact(ops, case, adj, L, "%s L=%d" % (setting, L))
    res["propagate"] = sorted(set(names))
    # test d's case: d = 64 (d = 128 for the forced dense first backward layer, which d = 64 takes by default)
    d = 128 if setting == "bwd1_dense" else 64
    step = sc.run_train_case(ops, d, ops.LOSS_RUBIBCEBOTH, env)
    res["step"] = sorted(set(step))
    if setting == "stream_fused":
        ok = res["propagate"] == ["spmm_stream"] and "spmm_stream+adam" in step and "spmm_csr+adam" not in step
    elif setting == "records0":
        ok = res["propagate"] == ["spmm_csr"] and "spmm_csr+adam" in step
    elif setting == "bwd1_sparse":
        ok = "spmm_csr_sparse" in step and "spmm_csr+adam" in step
    elif setting == "bwd1_dense":
        ok = "spmm_csr_sparse" not in step and "spmm_csr_rows" in step and "spmm_csr+adam" in step
    else:
        raise SystemExit("unknown setting %r" % setting)
    res["ok"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
