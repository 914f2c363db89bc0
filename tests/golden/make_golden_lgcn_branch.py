#!/usr/bin/env python3
"""G12: golden losses / gradients / rankings of LightGCN's item-branch losses, computed by the reference's own graph code.

    macr_lightgcn/LightGCN.py  create_bce_loss_two_brach1 (:432-461)  -- `--loss bce1`, rubi_ratings1 (:442)
                               create_bce_loss_two_brach2 (:463-493)  -- `--loss bce2`, rubi_ratings2 (:473)

executed as tests/golden/make_golden_model.py executes the other loss builders (its `tensorflow` stand-in and its problems
are imported, not copied) on G10's LightGCN cases a / b (this script checks the inputs against G10), in float32 and float64.
rubi_ratings1/2 are the builders' (B, B) test scores (batch_ratings - c) * sig(pos_item_scores) at c = C.  Only outputs are
stored (tests/golden/G12_lgcn_item_branch.npz): losses of both runs, gradients and scores of the float64 run.

Usage:  python tests/golden/make_golden_lgcn_branch.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_bpr as GB  # noqa: E402
import make_golden_model as G  # noqa: E402

C = 0.5
BUILDERS = {"bce1": ("create_bce_loss_two_brach1", "rubi_ratings1"), "bce2": ("create_bce_loss_two_brach2", "rubi_ratings2")}


def run(LightGCN, fn_name, ratings_name, prob, hyper, n_layers, dtype):
    """make_golden_model.run_lgcn with rubi_c = C, returning the builder's ranking tensor too"""
    pre, P, Q, w, wu, u, i, j = prob
    t = lambda a: torch.tensor(a, dtype=dtype, requires_grad=True)
    Pt, Qt, wt, wut = t(P), t(Q), t(w), t(wu)
    tf = sys.modules["tensorflow"]
    me = types.SimpleNamespace(n_users=P.shape[0], n_items=Q.shape[0], n_fold=100, norm_adj=pre, n_layers=n_layers,
                               node_dropout_flag=0, weights={"user_embedding": Pt, "item_embedding": Qt},
                               w=wt, w_user=wut, alpha=hyper["alpha"], beta=hyper["beta"], decay=hyper["decay"],
                               batch_size=hyper["batch_size"], rubi_c=torch.full((1,), C, dtype=dtype))
    me._convert_sp_mat_to_sp_tensor = lambda X: LightGCN._convert_sp_mat_to_sp_tensor(me, X)
    me._split_A_hat = lambda X: LightGCN._split_A_hat(me, X)
    ua, ia = LightGCN._create_lightgcn_embed(me)
    ui, ii, ji = torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(j)
    ug, pg, ng = (tf.nn.embedding_lookup(ua, ui), tf.nn.embedding_lookup(ia, ii), tf.nn.embedding_lookup(ia, ji))
    me.u_g_embeddings_pre = tf.nn.embedding_lookup(Pt, ui)
    me.pos_i_g_embeddings_pre = tf.nn.embedding_lookup(Qt, ii)
    me.neg_i_g_embeddings_pre = tf.nn.embedding_lookup(Qt, ji)
    me.batch_ratings = tf.matmul(ug, pg, transpose_a=False, transpose_b=True)
    mf_loss, emb_loss, reg_loss = getattr(LightGCN, fn_name)(me, ug, pg, ng)
    loss = mf_loss + emb_loss
    grads = torch.autograd.grad(loss, [Pt, Qt, wt, wut], allow_unused=True)
    z = lambda g, ref: np.zeros_like(ref) if g is None else g.detach().numpy()
    return {"loss": float(loss.detach()), "mf_loss": float(mf_loss.detach()), "emb_loss": float(emb_loss.detach()),
            "reg_loss": float(np.asarray(reg_loss.detach()).ravel()[0]),
            "dP": z(grads[0], P), "dQ": z(grads[1], Q), "dw": z(grads[2], w), "dwu": z(grads[3], wu),
            "ratings": getattr(me, ratings_name).detach().numpy()}


def main():
    _, LightGCN = GB.load_builders()
    g10 = {}
    for f in sorted(os.listdir(HERE)):
        if f.startswith("G10_model_steps_") and f.endswith(".npz"):
            with np.load(os.path.join(HERE, f)) as z:
                g10.update((k, z[k]) for k in z.files)
    out = {}
    for tag, (seed, nu, ni, d, B, n_inter) in GB.LGCN_CASES.items():
        prob = G.lgcn_problem(seed, nu, ni, d, B, n_inter)
        for k, v in zip(("P", "Q", "w", "wu", "u", "i", "j"), prob[1:]):
            assert np.array_equal(v, g10["lgcn_%s/%s" % (tag, k)]), (tag, k)
        assert np.array_equal(prob[0].data, g10["lgcn_%s/data" % tag])
        for loss, (fn, rname) in BUILDERS.items():
            for dt, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
                res = run(LightGCN, fn, rname, prob, GB.HYPER, 2, dt)
                for k, v in res.items():
                    if dname == "f64" or np.ndim(v) == 0:
                        out["lgcn_%s/%s/%s/%s" % (tag, loss, dname, k)] = np.asarray(v)
    out["hyper"] = np.asarray([GB.HYPER["alpha"], GB.HYPER["beta"], GB.HYPER["decay"], GB.HYPER["batch_size"], C], np.float64)
    path = os.path.join(HERE, "G12_lgcn_item_branch.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KB)" % (path, len(out), os.path.getsize(path) / 1024))
    for tag in GB.LGCN_CASES:
        for loss in BUILDERS:
            print("lgcn_%s %s loss f32 %.6f f64 %.6f" % (tag, loss, out["lgcn_%s/%s/f32/loss" % (tag, loss)],
                                                       out["lgcn_%s/%s/f64/loss" % (tag, loss)]))


if __name__ == "__main__":
    main()
