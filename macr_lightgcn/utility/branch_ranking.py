"""`test()` / `test_sweep()` of utility/batch_test.py, extended by LightGCN's one-branch rankings of the reference's test
dispatch (batch_test.py:66-84, LightGCN.py:848-854):
    rubi1  rubi_ratings1 (LightGCN.py:442): (y_ui - c) sigmoid(e_i . w), e_i the PROPAGATED item rows
    rubi2  rubi_ratings2 (LightGCN.py:473): the same with the branch factors of the EGO item rows (the scores still read the
           propagated ones)
Every other method goes to batch_test's own functions unchanged."""
import numpy as np
import torch

from utility import batch_test as _bt

from macr_amd import ops
from macr_amd.eval_cache import EvaluatorCache
from macr_amd.evaluator import Evaluator

# method -> whether the item branch reads the ego rows
_ITEM_BRANCH = {"rubi1": False, "rubi2": True}
_evaluators = EvaluatorCache(max_cached=4)


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
    """batch_test.test with the methods rubi1 / rubi2 as well"""
    if method not in _ITEM_BRANCH:
        return _bt.test(sess, model, users_to_test, drop_flag, train_set_flag, method)
    if train_set_flag != 0:
        raise NotImplementedError("train_set_flag != 0 is unused by the reference CLI")
    evaluator, uid = _evaluator_for(model, users_to_test)
    ua, ia = model.propagated()
    ret = evaluator.test_lgcn(ops.SCORE_RUBI, ua, uid, ia.contiguous(), model.Ks, model.w, model.w_user, model.rubi_c,
                              branch=_branch(model, method))
    return {k: np.asarray(v) for k, v in ret.items()}


def test_sweep(sess, model, users_to_test, cs, method="rubiboth"):
    """batch_test.test_sweep with the methods rubi1 / rubi2 as well"""
    if method not in _ITEM_BRANCH:
        return _bt.test_sweep(sess, model, users_to_test, cs, method)
    evaluator, uid = _evaluator_for(model, users_to_test)
    ua, ia = model.propagated()
    rets = evaluator.test_lgcn_sweep(ops.SCORE_RUBI, ua, uid, ia.contiguous(), model.Ks, model.w, model.w_user, list(cs),
                                     branch=_branch(model, method))
    return [{k: np.asarray(v) for k, v in r.items()} for r in rets]
