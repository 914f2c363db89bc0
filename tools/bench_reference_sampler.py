"""What `--sampler reference` costs: the native reference-stream sampler (macr_amd/host_sampler.py) against the Python form it
replaces (MFData.sample, LGCNData.sample), in one process, in triples per second.  No GPU needed for the rates.

    python tools/bench_reference_sampler.py                      # rates -> profiles/reference_sampler.json
    python tools/bench_reference_sampler.py --e2e [--parent DIR] # on an MI355X: + the README's two Addressa commands

Rates: Addressa (MF and LightGCN streams, B = 1024) and a Gowalla-shaped synthetic (macr_amd/synth.py, B = 4096).  Both forms
start from the same seed and their batches are compared, so a rate is never reported for a stream that differs.  The tool
exits non-zero when a native rate is below 10x the Python rate of the same run.

--e2e: wall time of the two Addressa commands of tools/e2e_addressa.sh at default flags (so: --sampler reference), each in a
process of its own, in this tree and -- with --parent DIR, a checkout of the parent commit with its libraries built -- in
that one, on the same box; and from a run of this tree with train_epoch and begin_pass timed from the inside, the share of
the epochs spent in begin_pass.  The result is merged into the same JSON file.
"""
import argparse
import collections
import json
import os
import platform
import random
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "reference_sampler.json")

E2E = {
    "mf": ["macr_mf/train.py", "--dataset", "addressa", "--batch_size", "1024", "--cuda", "0", "--saveID", "0",
           "--log_interval", "10", "--lr", "0.001", "--check_c", "1", "--c", "40", "--train", "rubibceboth", "--test", "rubi",
           "--alpha", "1e-3", "--beta", "1e-3"],
    "lgcn": ["macr_lightgcn/LightGCN.py", "--data_path", "data/", "--dataset", "addressa", "--verbose", "1", "--layer_size",
             "[64,64]", "--Ks", "[20]", "--loss", "bceboth", "--test", "rubiboth", "--c", "40", "--epoch", "2000",
             "--early_stop", "1", "--lr", "0.001", "--batch_size", "1024", "--gpu_id", "0", "--log_interval", "10",
             "--alpha", "1e-2", "--beta", "1e-3"],
}


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def addressa():
    import types
    from macr_amd.data import LGCNData, MFData
    a = types.SimpleNamespace(data_path=os.path.join(REPO, "data") + "/", dataset="addressa", batch_size=1024,
                              data_type="ori", model="mf", source="normal", valid_set="test")
    return MFData(a), LGCNData(a.data_path + a.dataset, a.batch_size, a)


def gowalla_shaped():
    """the two loaders' sampling fields over macr_amd/synth.py's Gowalla-shaped interaction lists (no files)"""
    from macr_amd import synth
    from macr_amd.data import LGCNData, MFData
    cfg = synth.WORKLOADS["gowalla"]
    n_users, n_items, B = cfg["n_users"], cfg["n_items"], cfg["batch"]
    lists = synth.interaction_lists(n_users, n_items, cfg["n_train"] / n_users, seed=4242)
    mf = object.__new__(MFData)
    mf.n_users, mf.n_items, mf.batch_size = n_users, n_items, B
    mf.users, mf.items = list(range(n_users)), list(range(n_items))
    mf.train_user_list = collections.defaultdict(list, enumerate(lists))
    mf._train_sets = {}
    lg = object.__new__(LGCNData)
    lg.n_users, lg.n_items, lg.batch_size = n_users, n_items, B
    lg.exist_users, lg.train_items, lg.test_set, lg._train_sets = list(range(n_users)), dict(enumerate(lists)), {}, {}
    return mf, lg


def rate(name, sampler, fn, B, n_python, n_native):
    random.seed(12345)
    np.random.seed(12345)
    fn()                                                    # (the Python form caches a set per user: warm a little)
    random.seed(12345)
    np.random.seed(12345)
    t0 = time.perf_counter()
    want = np.asarray([fn() for _ in range(n_python)], dtype=np.int32)
    t_py = time.perf_counter() - t0
    random.seed(12345)
    np.random.seed(12345)
    sampler.generate(2)
    random.seed(12345)
    np.random.seed(12345)
    t0 = time.perf_counter()
    got = sampler.generate(n_native)
    t_nat = time.perf_counter() - t0
    if not np.array_equal(got[:n_python], want):
        raise SystemExit("%s: the native batches differ from the Python form" % name)
    row = {"stream": name, "B": B, "python_batches": n_python, "native_batches": n_native,
           "python_triples_per_s": round(n_python * B / t_py), "native_triples_per_s": round(n_native * B / t_nat)}
    row["speedup"] = round(row["native_triples_per_s"] / row["python_triples_per_s"], 1)
    print(json.dumps(row))
    return row


def rates():
    from macr_amd.host_sampler import ReferenceStreamSampler as R
    rows = []
    mf, lg = addressa()
    rows.append(rate("addressa mf", R.for_mf(mf), mf.sample, 1024, 200, 2000))
    rows.append(rate("addressa lightgcn", R.for_lgcn(lg), lg.sample, 1024, 60, 2000))
    mf, lg = gowalla_shaped()
    rows.append(rate("gowalla-shaped mf", R.for_mf(mf), mf.sample, 4096, 40, 400))
    rows.append(rate("gowalla-shaped lightgcn", R.for_lgcn(lg), lg.sample, 4096, 12, 400))
    return rows


def timed_cli(which):
    """child process of --e2e: the CLI's main() with train_epoch and ReferenceStreamSampler.begin_pass timed"""
    from macr_amd import host_sampler
    spent = {"begin_pass_s": 0.0, "train_epoch_s": 0.0, "passes": 0, "epoch_calls": 0}
    inner = host_sampler.ReferenceStreamSampler.begin_pass

    def begin_pass(self, n):
        t0 = time.perf_counter()
        inner(self, n)
        spent["begin_pass_s"] += time.perf_counter() - t0
        spent["passes"] += 1
    host_sampler.ReferenceStreamSampler.begin_pass = begin_pass
    script = os.path.join(REPO, E2E[which][0])
    sys.argv = [script] + E2E[which][1:]
    sys.path.insert(0, os.path.dirname(script))
    import importlib
    cli = importlib.import_module(os.path.splitext(os.path.basename(script))[0])
    epoch = cli.train_epoch

    def train_epoch(*a, **kw):
        t0 = time.perf_counter()
        out = epoch(*a, **kw)
        spent["train_epoch_s"] += time.perf_counter() - t0
        spent["epoch_calls"] += 1
        return out
    cli.train_epoch = train_epoch
    cli.main()
    spent["begin_pass_share_of_train_epoch"] = round(spent["begin_pass_s"] / max(spent["train_epoch_s"], 1e-9), 4)
    print("E2E_SPENT " + json.dumps(spent))


def wall(cmd, cwd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=1500)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed in %s:\n%s" % (" ".join(cmd), cwd, (r.stdout + r.stderr)[-3000:]))
    return round(dt, 2), r.stdout


def e2e(parent):
    import tempfile
    import torch
    doc = {"gpu": torch.cuda.get_device_name(0), "cpu": cpu_model(), "commands": {}}
    for which, argv in E2E.items():
        row = {"argv": " ".join(argv)}
        for label, tree in (("this_commit", REPO), ("parent_commit", parent)):
            if tree is None:
                continue
            with tempfile.TemporaryDirectory() as tmp:          # (checkpoints and log files land in the working directory)
                os.symlink(os.path.join(REPO, "data"), os.path.join(tmp, "data"))
                row[label + "_wall_s"], out = wall([sys.executable, os.path.join(tree, argv[0])] + argv[1:], tmp)
                row[label + "_last_line"] = out.strip().splitlines()[-1][:200]
        with tempfile.TemporaryDirectory() as tmp:
            os.symlink(os.path.join(REPO, "data"), os.path.join(tmp, "data"))
            _, out = wall([sys.executable, os.path.abspath(__file__), "--timed-cli", which], tmp)
            row["inside"] = json.loads([l for l in out.splitlines() if l.startswith("E2E_SPENT ")][-1][len("E2E_SPENT "):])
        print(json.dumps({which: row}))
        doc["commands"][which] = row
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, libraries built, to time on the same box")
    ap.add_argument("--timed-cli", default=None, choices=sorted(E2E))
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.timed_cli:
        return timed_cli(a.timed_cli)
    have = a.out if os.path.exists(a.out) else OUT             # (--out elsewhere: the committed file is the starting point)
    doc = json.load(open(have)) if os.path.exists(have) else {}
    if a.e2e:
        doc["e2e_mi355x"] = e2e(os.path.abspath(a.parent) if a.parent else None)
    else:
        rows = rates()
        doc["rates"] = {"cpu": cpu_model(), "cpus": os.cpu_count(), "rows": rows,
                        "floor": "native >= 10x the Python form of the same run, every row"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if not a.e2e and any(r["native_triples_per_s"] < 10 * r["python_triples_per_s"] for r in doc["rates"]["rows"]):
        raise SystemExit("a native rate is below 10x the Python form")


if __name__ == "__main__":
    main()
