"""Full-catalogue positions on the GPU: macr_score_pairs / macr_rank_positions against oracle.score_matrix followed by integer
counting with the key rule (tests/rank_ref.py) -- positions EQUAL, scores bit-equal --, Evaluator.rank_positions against
Evaluator.rank (two independent kernels), the models' predict against rank()'s values, and the MACR_RANK_REPORT=1 line of
both command lines against a recomputation from the saved checkpoint."""
import ctypes
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import oracle
import rank_ref
from helpers import GOLD, REPO

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a5a5a5a
KINDS = ["SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_RUBI", "SCORE_DIRECT_MINUS", "SCORE_DIRECT_MINUS_BOTH"]
PAIR_LENS = (0, 1, 5, 17, 40)              # in one call; 17 and 40 lie on both sides of a cut at 16 and of one at 32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def csr_np(lists):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int32)
    idx = np.asarray([x for r in lists for x in r] or [0], dtype=np.int32)
    return ptr, idx


def raw(ops, kind, P, uid, Q, sig_u, sig_i, c, c_dev, mask, pairs):
    """both entry points through the C ABI on outputs and a workspace pre-filled with garbage -> (positions, scores)"""
    from macr_amd import _lib
    L = _lib.lib()
    U = len(pairs)
    n_local, d = Q.shape
    pp, pi = csr_np(pairs)
    n_pairs = int(pp[-1])
    pp, pi = dev(pp), dev(pi)
    mp = mi = None
    if mask is not None:
        mp, mi = (dev(a) for a in csr_np(mask))
    pos = torch.full((max(n_pairs, 1),), GARBAGE, dtype=torch.int32, device="cuda")
    sc = torch.full((max(n_pairs, 1),), float("inf"), dtype=torch.float32, device="cuda")
    need = L.macr_rank_positions_workspace_bytes(U, n_pairs, n_local, d)
    assert need > 0
    ws = torch.full((need,), 0x5a, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cv, cp = (0.0, p(c_dev)) if c_dev is not None else (float(c), None)
    _lib.check(L.macr_score_pairs(kind, U, n_local, d, p(P), p(uid), p(Q), p(sig_u), p(sig_i), cv, cp, p(pp), p(pi), n_pairs,
                                  p(sc), st))
    _lib.check(L.macr_rank_positions(kind, U, n_local, d, p(P), p(uid), p(Q), p(sig_u), p(sig_i), cv, cp, p(mp), p(mi), p(pp),
                                     p(pi), n_pairs, p(pos), p(ws), need, st))
    return pos.cpu().numpy()[:n_pairs], sc.cpu().numpy()[:n_pairs]


def tables(rs, n_tab, n_local, d):
    P = (rs.standard_normal((n_tab, d)) * 0.5).astype(np.float32)
    Q = (rs.standard_normal((n_local, d)) * 0.5).astype(np.float32)
    Q += (rs.standard_normal(n_local).astype(np.float32) * 0.5)[:, None] * np.sign(P.mean(0, keepdims=True))      # popularity
    w = (rs.standard_normal(d) * 0.3).astype(np.float32)
    wu = (rs.standard_normal(d) * 0.3).astype(np.float32)
    return P, Q, w, wu


def lists(rs, U, n_local, mask_lens=None):
    """pair lists of every length of PAIR_LENS (ids from a little outside [0, n_local) too), masks of length 0, 3 and
    n_local - 1, and every seventh query masks one of its own pair items"""
    pairs, mask = [], []
    pool = np.arange(-2, n_local + 3)
    for q in range(U):
        n = min(PAIR_LENS[q % len(PAIR_LENS)], len(pool))
        pairs.append(sorted(rs.choice(pool, n, replace=False).tolist()))
        m = (mask_lens or (0, 3, n_local - 1))[q % 3]
        row = set(rs.choice(n_local, m, replace=False).tolist())
        own = [g for g in pairs[q] if 0 <= g < n_local]
        if q % 7 == 3 and own:
            row.add(own[0])
        mask.append(sorted(row))
    return pairs, mask


def reference(kind_name, P, uid, Q, w, wu, c):
    """(scores (U,N) of the oracle, sig_u, sig_i as the oracle computes them)"""
    kind = getattr(oracle, kind_name)
    rows = P if uid is None else P[uid]
    sig_i = oracle.branch_sigmoid(Q, w) if kind_name != "SCORE_NORMAL" else None
    sig_u = oracle.branch_sigmoid(rows, wu) if kind_name.endswith("_BOTH") else None
    return oracle.score_matrix(kind, rows, Q, sig_u, sig_i, c), sig_u, sig_i


def check(ops, kind_name, P, uid, Q, w, wu, c, use_c_dev, mask, pairs):
    scores, sig_u, sig_i = reference(kind_name, P, uid, Q, w, wu, c)
    want_pos, want_sc = rank_ref.positions(scores, mask or [[]] * len(pairs), pairs), rank_ref.pair_scores(scores, pairs)
    c_dev = dev(np.asarray([c], dtype=np.float32)) if use_c_dev else None
    opt = lambda a: None if a is None else dev(a)
    pos, sc = raw(ops, getattr(ops, kind_name), dev(P), opt(uid), dev(Q), opt(sig_u), opt(sig_i), c, c_dev, mask, pairs)
    inside = ~np.isnan(want_sc)
    assert np.array_equal(sc.view(np.int32)[inside], want_sc.view(np.int32)[inside]), kind_name       # bit for bit
    assert np.all(np.isnan(sc[~inside]))
    assert np.array_equal(pos, want_pos), (kind_name, np.flatnonzero(pos != want_pos)[:10], pos[pos != want_pos][:10],
                                           want_pos[pos != want_pos][:10])
    return pos, want_pos


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("n_local", [31, 129, 333])        # below one tile, a tile edge + 1, ten tiles + 13
def test_positions_and_scores_equal_the_oracle(ops, n_local, d):
    rs = np.random.RandomState(1000 * n_local + d)
    U, n_tab = 37, 100
    P, Q, w, wu = tables(rs, n_tab, n_local, d)
    pairs, mask = lists(rs, U, n_local)
    perm = rs.permutation(n_tab)[:U].astype(np.int32)
    seen = set()
    for kind_name in KINDS:
        # a permutation into the 100-row table with c by value; the table's first rows as they are with c on the device
        pos, want = check(ops, kind_name, P, perm, Q, w, wu, 0.7, False, mask, pairs)
        check(ops, kind_name, P[:U].copy(), None, Q, w, wu, -1.3, True, mask, pairs)
        seen |= set(want.tolist())
    assert -1 in seen and max(seen) > min(n_local // 2, 100)
    # without a mask: only the ids outside the table have no position
    pos, _ = check(ops, "SCORE_RUBI_BOTH", P, perm, Q, w, wu, 0.7, False, None, pairs)
    flat = np.asarray([g for row in pairs for g in row])
    assert np.array_equal(pos == -1, (flat < 0) | (flat >= n_local))


def test_ties_are_broken_by_id(ops):
    rs = np.random.RandomState(5)
    U, n_local, d = 37, 129, 32
    P, Q, w, wu = tables(rs, U, n_local, d)
    pairs, mask = lists(rs, U, n_local)
    # an all-zero item table: every score is 0.0, a pair's position is the number of unmasked smaller ids
    pos, _ = check(ops, "SCORE_NORMAL", P, None, np.zeros_like(Q), w, wu, 0.0, False, mask, pairs)
    k = 0
    for q in range(U):
        for g in pairs[q]:
            if 0 <= g < n_local and g not in mask[q]:
                assert pos[k] == g - sum(1 for m in mask[q] if m < g), (q, g)
            else:
                assert pos[k] == -1
            k += 1
    # duplicated rows: seven distinct items repeated over the catalogue, also through the branch factors
    dup = Q[np.arange(n_local) % 7].copy()
    for kind_name in ("SCORE_NORMAL", "SCORE_RUBI_BOTH", "SCORE_DIRECT_MINUS"):
        check(ops, kind_name, P, None, dup, w, wu, 0.4, True, mask, pairs)
    # -0.0 and +0.0 tie, a NaN row ranks before nothing and has no position itself
    odd = Q.copy()
    odd[5] = 0.0
    odd[9] = -0.0
    odd[11] = np.nan
    pairs2 = [sorted(set(row) | {5, 9, 11}) for row in pairs]
    check(ops, "SCORE_NORMAL", P, None, odd, w, wu, 0.0, False, mask, pairs2)


def test_many_tiles_and_positions_above_2_16(ops):
    rs = np.random.RandomState(9)
    U, n_local, d = 8, 70001, 32
    P, Q, w, wu = tables(rs, U, n_local, d)
    pairs, mask = lists(rs, U, n_local, mask_lens=(0, 50, 3))
    pairs[7] = sorted(set(pairs[7]) | {n_local - 1, n_local - 33, 0})
    pos, _ = check(ops, "SCORE_RUBI_BOTH", P, None, Q, w, wu, 0.3, False, mask, pairs)
    assert pos.max() > 1 << 16
    check(ops, "SCORE_NORMAL", P, None, Q, w, wu, 0.0, False, mask, pairs)


# ----------------------------------------------------------------------------- the evaluator and the models
def _mf_model(rs, n_users, n_items, d=64):
    from macr_amd.mf import BPRMF
    P, Q, w, wu = tables(rs, n_users, n_items, d)
    args = types.SimpleNamespace(regs=1e-5, embed_size=d, lr=1e-3, batch_size=32, verbose=0, c=40.0, alpha=1e-2, beta=1e-3)
    return BPRMF(args, dict(n_users=n_users, n_items=n_items),
                 weights={"user_embedding": P, "item_embedding": Q, "w": w.reshape(-1, 1), "w_user": wu.reshape(-1, 1)})


def _lgcn_model(n_users, n_items):
    import scipy.sparse as sp
    from macr_amd.lightgcn import LightGCN
    rs = np.random.RandomState(3)
    n_inter = 6 * n_users
    R = sp.coo_matrix((np.ones(n_inter), (rs.randint(0, n_users, n_inter), rs.zipf(1.3, n_inter) % n_items)),
                      shape=(n_users, n_items)).tocsr()
    R = (R + sp.csr_matrix((np.ones(n_users), (np.arange(n_users), rs.randint(0, n_items, n_users))), shape=R.shape)).tocsr()
    R = (R + sp.csr_matrix((np.ones(n_items), (rs.randint(0, n_users, n_items), np.arange(n_items))), shape=R.shape)).tocsr()
    R.data[:] = 1.0
    A = sp.bmat([[None, R], [R.T, None]]).tocsr()
    deg = np.asarray(A.sum(1)).ravel()
    M = sp.diags(deg ** -0.5).dot(A).dot(sp.diags(deg ** -0.5)).tocsr().astype(np.float32)
    M.sort_indices()
    args = types.SimpleNamespace(adj_type="pre", alg_type="lightgcn", lr=1e-3, embed_size=64, batch_size=256,
                                 layer_size="[64,64]", regs="[1e-5]", verbose=0, Ks="[20]", alpha=1e-2, beta=1e-3,
                                 dataset="synthetic", node_dropout_flag=0)
    return LightGCN(dict(n_users=n_users, n_items=n_items, norm_adj=M), args, seed=3)


def _agree(ops, ev_lists, rank_args, rank_kw, predict, K=20):
    """every id rank() returns at index p gets position p from rank_positions, and predict() of (query, id) is rank()'s
    value bit for bit; twice on the same evaluator (the cached workspace)"""
    from macr_amd.evaluator import Evaluator
    mask, n_items, uid_np = ev_lists
    ev = Evaluator(mask, [[] for _ in mask], n_items, "cuda")
    val, idx, cnt = ev.rank(*rank_args, K, **rank_kw)
    idx_np, val_np = idx.cpu().numpy(), val.cpu().numpy()
    assert np.all(cnt.cpu().numpy() == K) and np.all(idx_np >= 0)
    gt = [sorted(row.tolist()) for row in idx_np]
    ev2 = Evaluator(mask, gt, n_items, "cuda")
    pos_kw = dict(rank_kw)
    first = ev2.rank_positions(*rank_args, **pos_kw)
    assert first.dtype == torch.int32 and first.shape == (len(mask) * K,) and first.is_cuda
    pos = first.cpu().numpy().reshape(len(mask), K)
    for q in range(len(mask)):
        # the CSR holds a query's ids ascending: slot j is the id whose index in the ranking is argsort(ids)[j]
        assert np.array_equal(pos[q], np.argsort(idx_np[q])), q
    again = ev2.rank_positions(*rank_args, **pos_kw)
    assert torch.equal(first, again)
    users = np.repeat(uid_np, K)
    got = predict(users, idx_np.reshape(-1)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), val_np.reshape(-1).view(np.int32))
    return ev2


@pytest.mark.parametrize("kind_name", ["SCORE_NORMAL", "SCORE_RUBI_BOTH"])
def test_evaluator_positions_agree_with_rank_mf(ops, kind_name):
    rs = np.random.RandomState(21)
    U, n_users, N = 300, 320, 2000
    model = _mf_model(rs, n_users, N)
    model.update_c(None, 0.7)
    kind = getattr(ops, kind_name)
    uid_np = rs.permutation(n_users)[:U].astype(np.int32)
    uid = dev(uid_np)
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(U)]
    ev = _agree(ops, (mask, N, uid_np), (kind, model.user_embedding, uid, model.item_embedding),
                dict(w=model.w, wu=model.w_user, c=model.rubi_c), lambda u, i: model.predict(kind, u, i))
    # the report on top of it: every pair is inside the first 20, so every percentile is small and the AUC near 1
    rep = ev.rank_report(kind, model.user_embedding, uid, model.item_embedding, model.w, model.w_user, model.rubi_c,
                         group_of=np.arange(N) % 6, n_groups=6)
    assert rep["users"] == U and rep["pairs"] == 20 * U and rep["skipped"] == 0 and rep["mrr"] == 1.0
    assert rep["group_pairs"].sum() == 20 * U and 0.99 < rep["auc"] <= 1.0
    # item-sharded evaluators have no position count yet
    ev.local_items_range = (0, N // 2)
    with pytest.raises(NotImplementedError):
        ev.rank_positions(kind, model.user_embedding, uid, model.item_embedding[:N // 2].contiguous(), model.w, model.w_user, 0.7)


def test_evaluator_positions_agree_with_rank_lightgcn_ego_branch(ops):
    rs = np.random.RandomState(22)
    n_users, N, U = 400, 2000, 300
    model = _lgcn_model(n_users, N)
    model.update_c(None, 0.02)
    ua, ia = model.propagated()
    ia = ia.contiguous()
    uid_np = rs.permutation(n_users)[:U].astype(np.int32)
    uid = dev(uid_np)
    mask = [sorted(rs.choice(N, rs.randint(0, 30), replace=False).tolist()) for _ in range(U)]
    _agree(ops, (mask, N, uid_np), (ops.SCORE_RUBI, ua, uid, ia),
           dict(w=model.w, wu=model.w_user, c=model.rubi_c, branch=model.ego_items()),
           lambda u, i: model.predict(model.RUBI_EGO, u, i))
    # predict on the propagated rows themselves is the matrix entry
    users, items = rs.randint(0, n_users, 50), rs.randint(0, N, 50)
    full = model.ratings(ops.SCORE_RUBI_BOTH, list(range(n_users)))
    got = model.predict(ops.SCORE_RUBI_BOTH, users, items)
    assert torch.equal(got, full[torch.as_tensor(users).cuda(), torch.as_tensor(items).cuda()])


# ----------------------------------------------------------------------------- CLIs on the tiny dataset
def _run(cmd, cwd, report):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.pop("MACR_RANK_REPORT", None)
    if report:
        env["MACR_RANK_REPORT"] = "1"
    out = subprocess.run([sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _recomputed_line(scores, train, test, n_items, train_counts):
    """the rank: line from a score matrix of the oracle, through tests/rank_ref.py and macr_amd/rank_report.py"""
    from macr_amd import popularity, rank_report
    test = [sorted(row) for row in test]
    pos = rank_ref.positions(scores, train, test)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in test])])
    idx = np.asarray([g for row in test for g in row])
    n_cand = np.asarray([n_items - len(set(row)) for row in train])
    rep = rank_report.summarize(pos, ptr, idx, n_cand, popularity.item_groups(train_counts), len(popularity.POINTS) + 1)
    return rank_report.format_line(rep)


def _rank_lines(out):
    return [l for l in out.splitlines() if l.startswith("rank: users=")]


def test_mf_cli_rank_report(ops, tmp_path):
    from macr_amd.data import MFData
    from macr_amd.mf import BPRMF
    on, off = tmp_path / "on", tmp_path / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    flags = lambda d: ["--data_path", str(d / "data") + "/", "--dataset", "tiny_data", "--batch_size", "16", "--cuda", "0",
                       "--saveID", "d", "--log_interval", "1", "--lr", "0.01", "--epoch", "3", "--train", "rubibceboth",
                       "--test", "rubi", "--c", "0.5", "--Ks", "[5, 20]", "--save_flag", "1", "--verbose", "1"]
    out1 = _run([os.path.join(REPO, "macr_mf", "train.py")] + flags(on), str(on), True)
    out0 = _run([os.path.join(REPO, "macr_mf", "train.py")] + flags(off), str(off), False)
    lines = _rank_lines(out1)
    assert len(lines) == 3 and "rank:" not in out0, out1                    # one per evaluation; none without the variable
    strip = lambda out: [re.sub(r"\[\d+\.\d+s( \+ \d+\.\d+s)?\]", "[t]", l) for l in out.splitlines() if "recall=[" in l]
    assert strip(out1) == strip(out0) and len(strip(out0)) == 3            # the evaluation itself is untouched
    args = _load(os.path.join(REPO, "macr_mf", "parse.py"), "mf_parse_for_rank_report").parse_args(flags(on))
    data = MFData(args)
    model = BPRMF(args, dict(n_users=data.n_users, n_items=data.n_items))
    ckpt = glob.glob(str(on / "*_checkpoint" / "*" / "2_ckpt.pt"))
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    assert model.rubi_c == 0.5
    users = list(data.test_user_list.keys())
    Pn, Qn = model.user_embedding.cpu().numpy(), model.item_embedding.cpu().numpy()
    sig_i = oracle.branch_sigmoid(Qn, model.w.cpu().numpy())
    sig_u = oracle.branch_sigmoid(Pn[users], model.w_user.cpu().numpy())
    scores = oracle.score_matrix(oracle.SCORE_RUBI_BOTH, Pn[users], Qn, sig_u, sig_i, 0.5)
    train, test = data.eval_lists(users)
    counts = [len(data.train_item_list.get(i, ())) for i in range(data.n_items)]
    assert lines[-1] == _recomputed_line(scores, train, test, data.n_items, counts)
    assert re.fullmatch(r"rank: users=\d+ pairs=\d+ skipped=\d+ auc=\d\.\d{5} mrr=\d\.\d{5} mpr=\d\.\d{5} \| train-popularity groups "
                        r"\(<10,<50,<100,<200,<500,>=500\): pairs=\[\d+(, \d+){5}\] mpr=\[[0-9.na, ]+\]", lines[-1]), lines[-1]


def test_mf_cli_refuses_the_report_on_row_shards(ops, tmp_path):
    shutil.copytree(os.path.join(GOLD, "tiny_data"), tmp_path / "data" / "tiny_data")
    env = dict(os.environ, MACR_RANK_REPORT="1")
    out = subprocess.run([sys.executable, os.path.join(REPO, "macr_mf", "train.py"), "--data_path", str(tmp_path / "data") + "/",
                          "--dataset", "tiny_data", "--batch_size", "16", "--epoch", "1", "--row_shard", "1"], cwd=str(tmp_path),
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "MACR_RANK_REPORT" in out.stderr and "--row_shard 1" in out.stderr, out.stderr[-2000:]


def test_lightgcn_cli_rank_report(ops, tmp_path):
    from macr_amd.data import LGCNData
    from macr_amd.lightgcn import LightGCN
    on, off = tmp_path / "on", tmp_path / "off"
    for d in (on, off):
        shutil.copytree(os.path.join(GOLD, "tiny_data"), d / "data" / "tiny_data")
    flags = lambda d: ["--data_path", str(d / "data") + "/", "--dataset", "tiny_data", "--verbose", "1", "--layer_size", "[64,64]",
                       "--Ks", "[5]", "--lr", "0.01", "--batch_size", "16", "--gpu_id", "0", "--epoch", "3", "--log_interval", "1",
                       "--weights_path", str(d) + "/", "--saveID", "d", "--loss", "bce", "--test", "normal"]
    out1 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(on), str(on), True)
    out0 = _run([os.path.join(REPO, "macr_lightgcn", "LightGCN.py")] + flags(off), str(off), False)
    lines = _rank_lines(out1)
    assert len(lines) == 3 and "rank:" not in out0, out1
    args = _load(os.path.join(REPO, "macr_lightgcn", "utility", "parser.py"), "lgcn_parser_for_rank_report").parse_args(flags(on))
    data = LGCNData(args.data_path + args.dataset, args.batch_size, args)
    model = LightGCN(dict(n_users=data.n_users, n_items=data.n_items, norm_adj=data.get_adj_mat()[3]), args)
    ckpt = glob.glob(str(on / "weights" / "**" / "weights_d-3.pt"), recursive=True)
    assert len(ckpt) == 1, ckpt
    model.load_state_dict(torch.load(ckpt[0], map_location=model.device))
    users = list(data.test_set.keys())
    ua, ia = model.propagated()
    scores = oracle.score_matrix(oracle.SCORE_NORMAL, ua.cpu().numpy()[users], ia.cpu().numpy())
    train, test = data.eval_lists(users)
    counts = np.zeros(data.n_items, dtype=np.int64)
    for items in data.train_items.values():
        np.add.at(counts, np.asarray(items, dtype=np.int64), 1)
    assert lines[-1] == _recomputed_line(scores, train, test, data.n_items, counts)
