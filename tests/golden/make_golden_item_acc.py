#!/usr/bin/env python3
"""Generate tests/golden/G15_item_acc.json by RUNNING THE REFERENCE's two test() functions.

Both build an `item_acc_list` per user batch -- for every item the share of its test interactions that landed in the
user's top-k among non-train items:
  macr_mf/train.py test() :261-277               k = 5, a local that is never returned or written
  macr_lightgcn/utility/batch_test.py :94-115    k = 20, written to Lightgcn_macr.txt (rewritten per user batch)
The harness is tests/golden/make_golden.py's (imported, not copied): the do-nothing `tensorflow`, the stub session that
serves rows of a fixed score matrix, the regenerable score matrices and the tiny dataset (40 users, 25 items, 30 test
users).  With --batch_size 64 all 30 test users fall into ONE user batch, so the dictionary of that batch is the whole
dictionary.  The LightGCN half keeps the file's content; the MF half reads the local out of test()'s frame when it returns
(sys.setprofile).  Score kinds `normal` and `popular` only: heapq.nlargest's order among equal scores is not the
evaluator's (score descending, id ascending), so every user's k+1 best non-train scores are asserted distinct.

The fixture holds the inputs' seeds and the two dictionaries as strings: data the reference computed, none of its text.

Usage:  python tests/golden/make_golden_item_acc.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

OUT = os.path.join(HERE, "G15_item_acc.json")
KINDS = {"normal": 100, "popular": 102}          # make_golden's seeds of the same kinds
BATCH = 64
K_MF, K_LGCN = 5, 20


def assert_distinct(full, users, train_of, k):
    """every user's k+1 best scores outside her train list differ pairwise"""
    for u in users:
        cand = np.setdiff1d(np.arange(full.shape[1]), np.asarray(train_of(u), dtype=np.int64))
        top = np.sort(full[u, cand])[::-1][:k + 1]
        assert len(np.unique(top)) == len(top), "user %d: tied scores among the best %d" % (u, k + 1)


def run_mf(out):
    G.install_common_shims()
    work = tempfile.mkdtemp(prefix="golden_item_acc_mf_")
    shutil.copytree(os.path.join(HERE, "tiny_data"), os.path.join(work, "data", "tiny"))
    os.chdir(work)
    sys.path.insert(0, os.path.join(G.REF, "macr_mf"))
    sys.argv = ["train.py", "--dataset", "tiny", "--batch_size", str(BATCH), "--Ks", "[5, 20]"]
    import train as ref_train                    # noqa: E402  (reference module)
    data = ref_train.data
    users = list(data.test_user_list.keys())
    assert len(users) // BATCH + 1 == 1
    code = ref_train.test.__code__
    res = {}
    for kind, seed in KINDS.items():
        full = G.score_matrix(kind, data.n_users, data.n_items, seed)
        assert_distinct(full, users, lambda u: data.train_user_list[u], K_MF)
        seen = []

        def profile(frame, event, arg):
            if event == "return" and frame.f_code is code:
                seen.append(dict(frame.f_locals["item_acc_list"]))
        sys.setprofile(profile)
        try:
            ref_train.test(G.StubSession(full), G.StubModel(), users, model_type="o")
        finally:
            sys.setprofile(None)
        assert len(seen) == 1 and len(seen[0]) == data.n_items
        res[kind] = str(seen[0])
    json.dump(res, open(out, "w"))
    shutil.rmtree(work, ignore_errors=True)


def run_lgcn(out):
    G.install_common_shims()
    lib = G.load_ref_lib()
    work = tempfile.mkdtemp(prefix="golden_item_acc_lgcn_")
    shutil.copytree(os.path.join(HERE, "tiny_data"), os.path.join(work, "tiny"))
    os.chdir(work)
    sys.path.insert(0, os.path.join(G.REF, "macr_lightgcn"))
    ev = types.ModuleType("evaluator")
    ev.eval_score_matrix_foldout = lambda s, t, k=20, thread_num=None: G.ref_eval_score_matrix_foldout(lib, s, t, k, thread_num)[0]
    sys.modules["evaluator"] = ev
    sys.argv = ["LightGCN.py", "--data_path", work + "/", "--dataset", "tiny", "--batch_size", str(BATCH),
                "--Ks", "[5, 20]", "--layer_size", "[64,64]"]
    import utility.batch_test as ref_bt          # noqa: E402  (reference module)
    dg = ref_bt.data_generator
    users = list(dg.test_set.keys())
    assert len(users) // BATCH + 1 == 1
    model = G.StubModel()
    model.Ks = [5, 20]
    res = {}
    for kind, seed in KINDS.items():
        full = G.score_matrix(kind, dg.n_users, dg.n_items, seed)
        assert_distinct(full, users, lambda u: dg.train_items.get(u, []), K_LGCN)
        if os.path.exists("Lightgcn_macr.txt"):
            os.remove("Lightgcn_macr.txt")
        ref_bt.test(G.StubSession(full), model, users, method="normal")
        res[kind] = open("Lightgcn_macr.txt").read()
    json.dump(res, open(out, "w"))
    shutil.rmtree(work, ignore_errors=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] in ("mf", "lgcn"):
        (run_mf if sys.argv[1] == "mf" else run_lgcn)(sys.argv[2])
        return
    subprocess.check_call(["make", "-C", os.path.join(G.REPO, "oracle"), "ref"])
    parts = {}
    tmp = tempfile.mkdtemp(prefix="golden_item_acc_")
    for half in ("mf", "lgcn"):             # one process per half: both import a module called `utility` / parse sys.argv
        part = os.path.join(tmp, half + ".json")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), half, part])
        parts[half] = json.load(open(part))
    shutil.rmtree(tmp, ignore_errors=True)
    fixture = {"dataset": "tiny_data", "batch_size": BATCH, "seeds": KINDS, "k": {"mf": K_MF, "lgcn": K_LGCN},
               "mf": parts["mf"], "lgcn": parts["lgcn"]}
    with open(OUT, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
