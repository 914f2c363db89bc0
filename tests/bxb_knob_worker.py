"""Worker of tests/test_gpu_bxb_forms.py::test_form_edges_under_the_launch_knobs: MACR_BXB_ROWS and MACR_BXB_NEUTRAL are latched
by the first training step of a process, so each setting gets a process of its own with the knob in its environment.  Runs the
setting's cases of tests/bxb_cases.py against the oracle (bxb_cases.run_on_gpu) and prints a JSON verdict with the complete
step's losses and the measured distances.

    python tests/bxb_knob_worker.py rows2 | rows4 | neutral0
"""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bxb_cases as bc  # noqa: E402


def main(setting):
    res = {"setting": setting, "env": {k: v for k, v in os.environ.items() if k.startswith("MACR_BXB_")}, "cases": {}, "ok": False}
    names = bc.WORKER_SETTINGS[setting]
    for name in names:                                      # this process's knobs are the ones the cases were laid out for
        assert res["env"] == bc.CASES[name]["env"], (res["env"], bc.CASES[name]["env"])
    from macr_amd import ops
    try:
        for name in names:
            res["cases"][name] = bc.run_on_gpu(ops, name, note=lambda s: print(s, file=sys.stderr))
        res["ok"] = True
    except AssertionError:
        res["error"] = traceback.format_exc()[-3000:]
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
