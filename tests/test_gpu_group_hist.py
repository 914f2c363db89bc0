"""macr_group_hist (the kernel behind MACR_CALIBRATION_REPORT) on the GPU against the plain-loop restatement
(tests/calibration_ref.py): every output array bit for bit, on output buffers pre-filled with garbage.  Shapes: the smallest at
which the kernel can go wrong -- row counts that are no multiple of the four rows of a workgroup, k at and past one chunk of 64
entries with a stride above k, CSR rows of 0, 1, 63, 64, 65 and 200 entries in one call, 1, 6 and 64 groups."""
import ctypes

import numpy as np
import pytest
import torch

import calibration_ref as R

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a
N_ITEMS = 1000
BIG = 2 ** 31 - 1


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dirty(n_bytes):
    return torch.full((max(n_bytes, 16),), GARBAGE, dtype=torch.uint8, device="cuda")


def raw_hist(ops, U, ids, group_of, n_groups, row_ptr=None, stride=0, k=0, gt=None, weight=None, n_items=N_ITEMS, wsum=True,
             null=(), wsum_offset=0):
    """macr_group_hist through the C ABI on garbage-filled outputs -> (return code, cnt, hit, wsum as NumPy; None where absent)"""
    from macr_amd import _lib
    rows, g = max(U, 1), max(n_groups, 1)
    tens = {"row_ptr": None if row_ptr is None else dev(np.asarray(row_ptr, dtype=np.int32)),
            "ids": dev(np.asarray(ids, dtype=np.int32).ravel() if len(ids) else np.zeros(1, dtype=np.int32)),
            "gt_ptr": None if gt is None else gt.ptr, "gt_idx": None if gt is None else gt.idx,
            "group_of": dev(np.asarray(group_of, dtype=np.int32)), "item_weight": None if weight is None else dev(np.asarray(weight, dtype=np.int32)),
            "cnt": dirty(rows * g * 4), "hit": None if gt is None else dirty(rows * g * 4), "wsum": dirty(rows * 16 + 16) if wsum else None}
    p = lambda name: None if name in null or tens[name] is None else ctypes.c_void_p(tens[name].data_ptr() + (wsum_offset if name == "wsum" else 0))
    rc = _lib.lib().macr_group_hist(U, p("row_ptr"), p("ids"), stride, k, p("gt_ptr"), p("gt_idx"), n_items, p("group_of"), n_groups,
                                    p("item_weight"), p("cnt"), p("hit"), p("wsum"), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = lambda name, dt: None if tens[name] is None else tens[name].cpu().numpy()
    cnt = host("cnt", None)[:rows * g * 4].view(np.int32).reshape(rows, g)
    hit = None if tens["hit"] is None else host("hit", None)[:rows * g * 4].view(np.int32).reshape(rows, g)
    ws = None if tens["wsum"] is None else host("wsum", None)[:rows * 16].view(np.int64).reshape(rows, 2)
    return rc, cnt, hit, ws, tens


def tables(seed, n_groups, big_weights=False):
    """group_of with -1 and n_groups among its values; weights up to 2^31 - 1 when asked for"""
    rs = np.random.RandomState(seed)
    group_of = rs.randint(0, n_groups, N_ITEMS).astype(np.int32)
    group_of[rs.choice(N_ITEMS, 40, replace=False)] = -1
    group_of[rs.choice(N_ITEMS, 40, replace=False)] = n_groups
    weight = rs.randint(0, 5000, N_ITEMS).astype(np.int32)
    if big_weights:
        weight[rs.choice(N_ITEMS, 700, replace=False)] = BIG
    return group_of, weight


def ground_truth(rs, rows, U):
    """every fourth row has none; the others hold the row's first and last valid id as their own first / last element where
    the draw allows, and strangers"""
    gt = []
    for u in range(U):
        valid = [int(x) for x in rows[u] if 0 <= x < N_ITEMS]
        if u % 4 == 3 or not valid:
            gt.append([])
            continue
        gt.append(sorted(set([min(valid), max(valid)] + [x for x in valid if rs.rand() < 0.3] + rs.randint(0, N_ITEMS, 3).tolist())))
    return gt


def ranking_case(seed, U, k, stride, n_groups):
    rs = np.random.RandomState(seed)
    ids = np.stack([rs.permutation(N_ITEMS)[:stride] for _ in range(U)]).astype(np.int32)      # the slots past k hold valid ids
    group_of, weight = tables(seed, n_groups)
    if U >= 5:
        ids[1, :k] = np.resize(np.flatnonzero(group_of == 0), k)               # a row whose ids are all in one group
        if k >= 3:
            ids[2, k // 2], ids[2, 0], ids[2, k - 1] = -1, N_ITEMS, BIG                    # skipped slots, -1 in the middle
        ids[4, :k] = -1                                                              # an empty list
    return ids, group_of, weight, ground_truth(rs, ids[:, :k], U)


RANKING = [(1, 1, 2, 1), (5, 1, 4, 6), (1, 20, 32, 6), (5, 20, 32, 6), (7, 20, 21, 64), (7, 64, 80, 6), (5, 65, 128, 6), (7, 128, 130, 64),
           (259, 20, 32, 6), (5, 128, 129, 1)]


def check(got, want, names):
    for g, w, name in zip(got, want, names):
        if w is None:
            assert g is None, name
            continue
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("U,k,stride,n_groups", RANKING)
def test_ranking_form_bit_for_bit(ops, U, k, stride, n_groups):
    ids, group_of, weight, gt = ranking_case(1000 * U + k + n_groups, U, k, stride, n_groups)
    want = R.group_hist(ids, group_of, n_groups, N_ITEMS, gt, weight, k=k)
    csr = ops.CSR.from_lists(gt, "cuda")
    rc, cnt, hit, ws, _ = raw_hist(ops, U, ids, group_of, n_groups, stride=stride, k=k, gt=csr, weight=weight)
    assert rc == 0
    check((cnt, hit, ws), want, ("cnt", "hit", "wsum"))
    again = raw_hist(ops, U, ids, group_of, n_groups, stride=stride, k=k, gt=csr, weight=weight)            # two calls, the same bytes
    check(again[1:4], (cnt, hit, ws), ("cnt", "hit", "wsum"))
    # without ground truth, without weights, without wsum
    rc, cnt2, hit2, ws2, _ = raw_hist(ops, U, ids, group_of, n_groups, stride=stride, k=k)
    assert rc == 0 and hit2 is None
    check((cnt2,), want[:1], ("cnt",))
    assert np.array_equal(ws2[:, 1], want[2][:, 1]) and (ws2[:, 0] == 0).all()
    rc, cnt3, _, ws3, _ = raw_hist(ops, U, ids, group_of, n_groups, stride=stride, k=k, wsum=False)
    assert rc == 0 and ws3 is None
    check((cnt3,), want[:1], ("cnt",))
    # the torch face
    t = ops.group_hist(dev(ids), dev(group_of), n_groups, N_ITEMS, k=k, gt=csr, item_weight=dev(weight))
    assert t[0].dtype == t[1].dtype == torch.int32 and t[2].dtype == torch.int64 and t[0].shape == (U, n_groups) and t[2].shape == (U, 2)
    check([x.cpu().numpy() for x in t], want, ("cnt", "hit", "wsum"))
    if U >= 5:                                         # the hand-made rows are what they claim
        assert np.count_nonzero(cnt[1]) == 1 and cnt[1].sum() == k
        assert (cnt[4] == 0).all() and tuple(ws[4]) == (0, 0)
        assert k < 3 or ws[2, 1] == k - 3
        assert hit.sum() > 0
    if U >= 200:
        assert (hit.sum(axis=1)[np.arange(U) % 4 == 3] == 0).all() and cnt.sum() < ws[:, 1].sum()      # ids outside every group exist


def csr_case(seed, lengths, n_groups, big_weights=True):
    rs = np.random.RandomState(seed)
    rows = [rs.choice(N_ITEMS, n, replace=n > N_ITEMS).astype(np.int64).tolist() for n in lengths]
    for row in rows:
        if len(row) >= 63:
            row[len(row) // 2], row[0], row[-1] = -1, N_ITEMS, BIG
    group_of, weight = tables(seed, n_groups, big_weights)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    flat = np.array([x for r in rows for x in r], dtype=np.int64).astype(np.int32)
    return rows, ptr, flat, group_of, weight


@pytest.mark.parametrize("lengths,n_groups", [((0, 1, 63, 64, 65, 200, 0), 6), ((200,), 64), ((0,), 1), ((64, 0, 0, 65, 1), 1),
                                              ((65, 200, 63, 1, 0, 64, 129, 128, 2000), 64)])
def test_csr_form_bit_for_bit(ops, lengths, n_groups):
    rows, ptr, flat, group_of, weight = csr_case(len(lengths) * 100 + n_groups, lengths, n_groups)
    U = len(rows)
    gt = ground_truth(np.random.RandomState(3), rows, U)
    want = R.group_hist(rows, group_of, n_groups, N_ITEMS, gt, weight)
    if 200 in lengths:
        assert want[2][:, 0].max() > 2 ** 32                     # the sum of a 200-entry row needs 64 bits
    csr = ops.CSR.from_lists(gt, "cuda")
    rc, cnt, hit, ws, _ = raw_hist(ops, U, flat, group_of, n_groups, row_ptr=ptr, gt=csr, weight=weight)
    assert rc == 0
    check((cnt, hit, ws), want, ("cnt", "hit", "wsum"))
    rc, cnt2, hit2, ws2, _ = raw_hist(ops, U, flat, group_of, n_groups, row_ptr=ptr, weight=weight)        # the profile's form: no gt
    assert rc == 0 and hit2 is None
    check((cnt2, ws2), (want[0], want[2]), ("cnt", "wsum"))
    t = ops.group_hist(ops.CSR(dev(ptr), dev(flat if len(flat) else np.zeros(1, dtype=np.int32))), dev(group_of), n_groups, N_ITEMS,
                       item_weight=dev(weight))
    assert t[1] is None
    check((t[0].cpu().numpy(), t[2].cpu().numpy()), (want[0], want[2]), ("cnt", "wsum"))


def test_every_refusal_leaves_the_outputs_untouched(ops):
    from macr_amd import _lib
    ids, group_of, weight, gt = ranking_case(3, 5, 20, 32, 6)
    csr = ops.CSR.from_lists(gt, "cuda")
    base = dict(U=5, ids=ids, group_of=group_of, n_groups=6, stride=32, k=20, gt=csr, weight=weight)
    cases = [dict(U=0), dict(U=-1), dict(n_items=0), dict(n_items=-1), dict(n_groups=0), dict(n_groups=65), dict(k=0), dict(k=33),
             dict(row_ptr=np.arange(6) * 32), dict(row_ptr=np.arange(6) * 32, stride=0), dict(row_ptr=np.arange(6) * 32, k=0),
             dict(null=("ids",)), dict(null=("group_of",)), dict(null=("cnt",)), dict(null=("hit",)), dict(null=("gt_ptr",)),
             dict(null=("gt_idx",)), dict(null=("hit", "gt_ptr")), dict(wsum_offset=8)]
    for case in cases:
        rc, cnt, hit, ws, tens = raw_hist(ops, **dict(base, **case))
        assert rc == _lib.E_INVALID and b"group_hist" in _lib.lib().macr_last_error(), case
        for name in ("cnt", "hit", "wsum"):
            assert (tens[name].cpu().numpy() == GARBAGE).all(), (case, name)
    with pytest.raises(ops.MacrError):
        ops.group_hist(dev(ids), dev(group_of), 6, N_ITEMS, gt=ops.CSR.from_lists(gt[:4], "cuda"))
    with pytest.raises(ops.MacrError):
        ops.group_hist(dev(ids), dev(group_of[:-1]), 6, N_ITEMS)
    with pytest.raises(ops.MacrError):
        ops.group_hist(dev(ids), dev(group_of), 6, N_ITEMS, k=33)
