"""`test()` / `test_sweep()` of utility/batch_test.py, extended by LightGCN's one-branch rankings of the reference's test
dispatch (batch_test.py:66-84, LightGCN.py:848-854):
    rubi1  rubi_ratings1 (LightGCN.py:442): (y_ui - c) sigmoid(e_i . w), e_i the PROPAGATED item rows
    rubi2  rubi_ratings2 (LightGCN.py:473): the same with the branch factors of the EGO item rows (the scores still read the
           propagated ones)
Every other method goes to batch_test's own functions unchanged.  Under --out 1 every test() is followed by the reference's
per-item diagnostic of the same ranking (batch_test.py:94-115), item_diagnostic below."""
import numpy as np
import torch

from utility import batch_test as _bt

from macr_amd import calibration, exposure, ops, popularity, rank_report, sharding, shift_report
from macr_amd.eval_cache import EvaluatorCache
from macr_amd.evaluator import Evaluator

# method -> whether the item branch reads the ego rows
_ITEM_BRANCH = {"rubi1": False, "rubi2": True}
_evaluators = EvaluatorCache(max_cached=4)
ITEM_ACC_K, ITEM_ACC_FILE = 20, "Lightgcn_macr.txt"       # heapq.nlargest(20, ...) and the file of batch_test.py:110-115
_popularity = {}


def _evaluator_for(model, users_to_test):
    """(Evaluator, device user ids) of this user list; built once per list (macr_amd/eval_cache.py)"""
    def build(users):
        mask, gt = _bt.data_generator.eval_lists(users)
        return (Evaluator(mask, gt, _bt.ITEM_NUM, model.device),
                torch.tensor(list(users), dtype=torch.int32, device=model.device))
    return _evaluators.get("test", users_to_test, build)


def _branch(model, method):
    return model.ego_items() if _ITEM_BRANCH[method] else None


def test(sess, model, users_to_test, drop_flag=False, train_set_flag=0, method="normal"):
    """batch_test.test with the methods rubi1 / rubi2 as well, and with --out 1 the item diagnostic of the same ranking"""
    if method not in _ITEM_BRANCH:
        ret = _bt.test(sess, model, users_to_test, drop_flag, train_set_flag, method)
    else:
        if train_set_flag != 0:
            raise NotImplementedError("train_set_flag != 0 is unused by the reference CLI")
        evaluator, uid = _evaluator_for(model, users_to_test)
        ua, ia = model.propagated()
        ret = evaluator.test_lgcn(ops.SCORE_RUBI, ua, uid, ia.contiguous(), model.Ks, model.w, model.w_user, model.rubi_c,
                                  branch=_branch(model, method))
        ret = {k: np.asarray(v) for k, v in ret.items()}
    if _bt.args.out == 1:
        item_diagnostic(sess, model, users_to_test, method)
    if rank_report.wanted():
        rank_diagnostic(sess, model, users_to_test, method)
    if exposure.enabled():
        exposure_diagnostic(sess, model, users_to_test, method)
    if shift_report.enabled() and method != "normal":
        shift_diagnostic(sess, model, users_to_test, method)
    if calibration.enabled():
        calibration_diagnostic(sess, model, users_to_test, method)
    return ret


def _popularity_tables():
    """{'group_of': the popularity group of every item, 'n_test': its test interactions, 'train_counts': its train
    interactions}, built once"""
    if not _popularity:
        data = _bt.data_generator
        counts = np.zeros(_bt.ITEM_NUM, dtype=np.int64)
        for items in data.train_items.values():
            np.add.at(counts, np.asarray(items, dtype=np.int64), 1)
        n_test = np.zeros(_bt.ITEM_NUM, dtype=np.int64)
        for item, users in data.test_item_set.items():
            n_test[item] = len(users)
        _popularity.update(group_of=popularity.item_groups(counts), n_test=n_test, train_counts=counts)
    return _popularity


def rank_diagnostic(sess, model, users_to_test, method):
    """MACR_RANK_REPORT=1: one line on where the held-out items stand in the FULL ranking test() scores with the same arguments
    (same score kind, the model's current c -- after a sweep the chosen one): AUC, reciprocal rank and rank percentile over
    the whole catalogue, overall and per train-popularity group of --out 1 (macr_amd/rank_report.py).  MACR_SHARD_RANK_REPORT=1:
    the same line counted over item shards -- every rank counts its items, the counts are added.  The main rank prints."""
    one_branch = method in _ITEM_BRANCH
    evaluator, uid = (_evaluator_for if one_branch else _bt._evaluator_for)(model, users_to_test)
    kind = ops.SCORE_RUBI if one_branch else _bt._METHODS[method]
    ua, ia = model.propagated()
    report = evaluator.rank_report_sharded if rank_report.shard_enabled() else evaluator.rank_report
    rep = report(kind, ua, uid, ia.contiguous(), model.w, model.w_user, model.rubi_c,
                 branch=_branch(model, method) if one_branch else None,
                 group_of=_popularity_tables()["group_of"], n_groups=len(popularity.POINTS) + 1)
    if sharding.is_main():
        print(rank_report.format_line(rep))


def exposure_diagnostic(sess, model, users_to_test, method):
    """MACR_EXPOSURE_REPORT=1: one line on the concentration of the top-max(Ks) lists test() ranks with the same arguments (same
    score kind, the model's current c -- after a sweep the chosen one): catalogue coverage, Gini, average recommendation
    popularity, each also with every slot weighted by 1 / log2(position + 2), and the train-popularity groups' shares of
    that exposure and of the DCG mass of the hits (macr_amd/exposure.py).  Every rank ranks; the main rank prints."""
    one_branch = method in _ITEM_BRANCH
    evaluator, uid = (_evaluator_for if one_branch else _bt._evaluator_for)(model, users_to_test)
    kind = ops.SCORE_RUBI if one_branch else _bt._METHODS[method]
    tables = _popularity_tables()
    k, n_groups = max(model.Ks), len(popularity.POINTS) + 1
    ua, ia = model.propagated()
    rec, exp_w, hit_w, _ = evaluator.item_exposure(kind, ua, uid, ia.contiguous(), k, model.w, model.w_user, model.rubi_c,
                                                   branch=_branch(model, method) if one_branch else None,
                                                   group_of=tables["group_of"], n_groups=n_groups)
    if sharding.is_main():
        print(exposure.format_line(exposure.summarize(rec.cpu().numpy(), exp_w.cpu().numpy(), hit_w.cpu().numpy(),
                                                      tables["train_counts"], tables["group_of"], n_groups, len(users_to_test), k)))


def shift_diagnostic(sess, model, users_to_test, method):
    """MACR_SHIFT_REPORT=1: one line on what the correction changed, user by user -- the top-max(Ks) lists test() ranks with the
    same arguments (same score kind, the model's current c -- after a sweep the chosen one) against the lists of the factual
    ranking (--test normal): how much of the lists was replaced and how high up, the hits kept, gained and lost on the same
    users with the exact sign test, and the train-popularity groups the replaced slots went to and came from
    (macr_amd/shift_report.py).  =2 adds the full-catalogue depth of the items that entered and left.  Every rank ranks; the
    main rank prints."""
    one_branch = method in _ITEM_BRANCH
    evaluator, uid = (_evaluator_for if one_branch else _bt._evaluator_for)(model, users_to_test)
    kind = ops.SCORE_RUBI if one_branch else _bt._METHODS[method]
    group_of = _popularity_tables()["group_of"]
    k, n_groups = max(model.Ks), len(popularity.POINTS) + 1
    ua, ia = model.propagated()
    tables, branch = (kind, ua, uid, ia.contiguous()), _branch(model, method) if one_branch else None
    per_user, entered, left, (e_rec, e_hit, _), (l_rec, l_hit, _) = evaluator.list_shift(
        *tables, k, model.w, model.w_user, model.rubi_c, branch=branch, group_of=group_of, n_groups=n_groups)
    depth = None
    if shift_report.enabled() == 2:
        depth = [p.cpu().numpy() for p in evaluator.shift_depth(*tables, entered, left, model.w, model.w_user, model.rubi_c, branch=branch)]
    if sharding.is_main():
        print(shift_report.format_line(shift_report.summarize(per_user.cpu().numpy(), e_rec.cpu().numpy(), e_hit.cpu().numpy(),
                                                              l_rec.cpu().numpy(), l_hit.cpu().numpy(), group_of, n_groups, k, depth)))


def calibration_diagnostic(sess, model, users_to_test, method):
    """MACR_CALIBRATION_REPORT=1: one line on whether the top-max(Ks) lists test() ranks with the same arguments (same score
    kind, the model's current c -- after a sweep the chosen one) follow each user's own taste for popularity: the divergence
    between the train-popularity mix of the user's profile and of its list (Jensen-Shannon, total variation), the popularity
    lift of the lists over the profiles, and both with the recall for the niche, diverse and blockbuster-minded users
    (macr_amd/calibration.py).  =2 adds the same figures of the factual ranking (--test normal) on the same users.  Every
    rank ranks; the main rank prints."""
    one_branch = method in _ITEM_BRANCH
    evaluator, uid = (_evaluator_for if one_branch else _bt._evaluator_for)(model, users_to_test)
    kind = ops.SCORE_RUBI if one_branch else _bt._METHODS[method]
    tables = _popularity_tables()
    k, n_groups = max(model.Ks), len(popularity.POINTS) + 1
    ua, ia = model.propagated()
    profile, here, base = evaluator.list_calibration(
        kind, ua, uid, ia.contiguous(), k, model.w, model.w_user, model.rubi_c, branch=_branch(model, method) if one_branch else None,
        group_of=tables["group_of"], n_groups=n_groups, item_weight=tables["train_counts"],
        with_base=calibration.enabled() == 2 and kind != ops.SCORE_NORMAL)
    if sharding.is_main():
        host = lambda t: None if t is None else [x.cpu().numpy() for x in t]
        print(calibration.format_line(calibration.summarize(host(profile), host(here), np.diff(evaluator.gt.ptr.cpu().numpy()), k,
                                                            host(base))))


def item_diagnostic(sess, model, users_to_test, method):
    """--out 1: the item_acc_list of batch_test.py:94-115 for the ranking test() scores with the same arguments (same score
    kind, the model's current c -- after a sweep the chosen one), written to Lightgcn_macr.txt as the reference writes it,
    and one line on the six popularity groups (the cut of macr_mf/load_data.py:424-466 on this loader's train lists).
    Every rank ranks; the main rank writes and prints."""
    one_branch = method in _ITEM_BRANCH
    evaluator, uid = (_evaluator_for if one_branch else _bt._evaluator_for)(model, users_to_test)
    kind = ops.SCORE_RUBI if one_branch else _bt._METHODS[method]
    _popularity_tables()
    ua, ia = model.propagated()
    rec, hit, sums = evaluator.item_accuracy(kind, ua, uid, ia.contiguous(), ITEM_ACC_K, model.w, model.w_user, model.rubi_c,
                                             branch=_branch(model, method) if one_branch else None,
                                             group_of=_popularity["group_of"], n_groups=len(popularity.POINTS) + 1)
    if sharding.is_main():
        popularity.emit(rec, hit, sums, _popularity["n_test"], _popularity["group_of"], ITEM_ACC_K, ITEM_ACC_FILE)


def test_sweep(sess, model, users_to_test, cs, method="rubiboth"):
    """batch_test.test_sweep with the methods rubi1 / rubi2 as well"""
    if method not in _ITEM_BRANCH:
        return _bt.test_sweep(sess, model, users_to_test, cs, method)
    evaluator, uid = _evaluator_for(model, users_to_test)
    ua, ia = model.propagated()
    rets = evaluator.test_lgcn_sweep(ops.SCORE_RUBI, ua, uid, ia.contiguous(), model.Ks, model.w, model.w_user, list(cs),
                                     branch=_branch(model, method))
    return [{k: np.asarray(v) for k, v in r.items()} for r in rets]
