"""macr_item_exposure on the GPU against the NumPy restatement (tests/exposure_ref.py) and, with unit weights, against
macr_item_counts.  Outputs and workspace are pre-filled with garbage; every comparison is exact integer equality."""
import ctypes

import numpy as np
import pytest
import torch

import exposure_ref as R

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_exposure(ops, rankings, gt_lists, weights, n_items, group_np=None, n_groups=0, with_out=True, raw_bytes=False):
    """macr_item_exposure through the C ABI on outputs and a workspace pre-filled with garbage
    -> (exp_w, hit_w, group sums or None) as NumPy int64"""
    from macr_amd import _lib
    U, K = rankings.shape
    rk = rankings if torch.is_tensor(rankings) else dev(rankings.astype(np.int32))
    gt = gt_lists if isinstance(gt_lists, ops.CSR) else ops.CSR.from_lists(gt_lists, "cuda")
    w = dev(np.asarray(weights, dtype=np.uint32).view(np.int32))
    L = _lib.lib()
    need = L.macr_item_exposure_workspace_bytes(U, K, n_items)
    assert need == _lib.ITEM_EXPOSURE_REPLICAS * n_items * 16
    fill = lambda n: torch.full((8 * n,), GARBAGE, dtype=torch.uint8, device="cuda").view(torch.int64)
    exp_w, hit_w = fill(n_items), fill(n_items)
    ws = torch.full((need,), GARBAGE, dtype=torch.uint8, device="cuda")
    group_of = None if group_np is None else dev(group_np.astype(np.int32))
    sums = fill(2 * n_groups) if group_np is not None and with_out else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(L.macr_item_exposure(U, K, len(weights), p(rk), p(gt.ptr), p(gt.idx), p(w), n_items, p(group_of), n_groups,
                                    p(exp_w), p(hit_w), p(sums), p(ws), need, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if raw_bytes:
        return exp_w.cpu().numpy().tobytes(), hit_w.cpu().numpy().tobytes(), sums.cpu().numpy().tobytes()
    return exp_w.cpu().numpy(), hit_w.cpu().numpy(), None if sums is None else sums.cpu().numpy().reshape(n_groups, 2)


def check(ops, rankings, gt, weights, n_items, group_np=None, n_groups=0, with_out=True):
    want_e, want_h = R.item_exposure(rankings, gt, weights, n_items)
    e, h, s = raw_exposure(ops, rankings, gt, weights, n_items, group_np, n_groups, with_out)
    assert e.dtype == np.int64 and np.array_equal(e, want_e) and np.array_equal(h, want_h)
    if group_np is not None and with_out:
        assert np.array_equal(s, R.group_sums(group_np, want_e, want_h, n_groups))
    else:
        assert s is None
    return want_e, want_h


def test_one_entry(ops):
    w = [12345]
    for gt, hit in (([[3]], 12345), ([[2, 4]], 0), ([[]], 0)):
        e, h = check(ops, np.array([[3]], dtype=np.int32), gt, w, 5)
        assert e.tolist() == [0, 0, 0, 12345, 0] and h.tolist() == [0, 0, 0, hit, 0]
    e, h = check(ops, np.array([[-1]], dtype=np.int32), [[0]], w, 5)
    assert not e.any() and not h.any()


@pytest.fixture(scope="module")
def small():
    """U = 37, K = 7, k = 3 over 50 items: -1 slots and ids >= n_items in the counted columns, ground-truth lists of length
    0, 1 and 9 (some holding ranked ids), one group id out of range"""
    rs = np.random.RandomState(37)
    U, K, n_items = 37, 7, 50
    rankings = np.stack([rs.permutation(n_items)[:K] for _ in range(U)]).astype(np.int32)
    rankings[rs.random_sample((U, K)) < 0.15] = -1
    rankings[rs.random_sample((U, K)) < 0.1] = n_items + rs.randint(0, 5)
    rankings[3, :3] = [-1, n_items, 2 ** 31 - 1]
    gt = []
    for u in range(U):
        n = (0, 1, 9)[u % 3]
        mine = [int(i) for i in rankings[u, :n] if 0 <= i < n_items]
        rest = [int(i) for i in rs.permutation(n_items) if i not in mine]
        gt.append(sorted(mine + rest[:n - len(mine)]))
    assert sorted(set(len(g) for g in gt)) == [0, 1, 9]
    return rankings, gt, n_items, rs


def test_small_shape_with_skips_and_groups(ops, small):
    rankings, gt, n_items, rs = small
    w = R.weights(3)
    want_e, want_h = check(ops, rankings, gt, w, n_items)
    assert want_h.any() and want_e.sum() > want_h.sum()
    assert want_e.sum() < int(w.astype(np.int64).sum()) * 37            # some entries were skipped
    for n_groups in (1, 64):
        group_np = rs.randint(0, n_groups, n_items).astype(np.int32)
        group_np[int(np.argmax(want_e))] = n_groups                      # out of range: in no group's sum
        check(ops, rankings, gt, w, n_items, group_np, n_groups)
        check(ops, rankings, gt, w, n_items, group_np, n_groups, with_out=False)     # group_out NULL: no group sums
    # the torch face
    gt_csr = ops.CSR.from_lists(gt, "cuda")
    group_np = (np.arange(n_items) % 6).astype(np.int32)
    e, h, s = ops.item_exposure(dev(rankings), gt_csr, w, n_items, dev(group_np), 6)
    assert e.dtype == h.dtype == s.dtype == torch.int64 and s.shape == (6, 2)
    assert np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(h.cpu().numpy(), want_h)
    assert np.array_equal(s.cpu().numpy(), R.group_sums(group_np, want_e, want_h, 6))
    e, h, s = ops.item_exposure(dev(rankings), gt_csr, w, n_items)
    assert s is None and np.array_equal(e.cpu().numpy(), want_e)


def hot_item(k):
    """U = 3000 lists of 4: item 7 at position u % 4, three ids of 40 others elsewhere; every third user holds item 7"""
    rs = np.random.RandomState(7)
    U = 3000
    others = np.setdiff1d(np.arange(8, 60), [13])[:40]
    rankings = np.empty((U, 4), dtype=np.int32)
    for u in range(U):
        row = rs.choice(others, 3, replace=False).tolist()
        row.insert(u % 4 if k == 4 else 0, 7)
        rankings[u] = row
    gt = [[7] if u % 3 == 0 else [int(rankings[u, ((u % 4 if k == 4 else 0) + 1) % 4])] for u in range(U)]
    return rankings, gt


def test_hot_item_across_workgroups_and_replicas(ops):
    from macr_amd import _lib
    rankings, gt = hot_item(4)
    tiles = -(-rankings.size // _lib.ITEM_EXPOSURE_TILE)
    assert tiles == 12 > _lib.ITEM_EXPOSURE_REPLICAS                    # one counter copy receives several workgroups' adds
    w = R.weights(4)
    group_np = (np.arange(60) % 6).astype(np.int32)
    want_e, want_h = check(ops, rankings, gt, w, 60, group_np, 6)
    assert want_e[7] == 750 * int(w.astype(np.int64).sum())
    assert want_h[7] == sum(int(w[u % 4]) for u in range(0, 3000, 3))


def test_sums_carry_past_32_bits(ops):
    rankings, gt = hot_item(1)
    assert (rankings[:, 0] == 7).all()
    w = np.array([2 ** 31], dtype=np.uint32)
    want_e, want_h = check(ops, rankings, gt, w, 60, np.zeros(60, dtype=np.int32), 1)
    assert want_e[7] == 3000 * 2 ** 31 > 2 ** 32 and want_h[7] == 1000 * 2 ** 31 > 2 ** 32
    w = np.array([2 ** 32 - 1], dtype=np.uint32)                         # the largest weight: no sign anywhere
    want_e, _ = check(ops, rankings, gt, w, 60)
    assert want_e[7] == 3000 * (2 ** 32 - 1)


def test_table_overflow_by_pigeonhole(ops):
    """2^22 entries with id(u, p) = (16 u + p) mod 2^20: a workgroup's contiguous share holds only distinct ids and more of
    them than its table has slots, so every workgroup sends entries down the cold path"""
    from macr_amd import _lib
    U, K, n_items = 2 ** 18, 16, 2 ** 20
    entries = U * K
    tiles = -(-entries // _lib.ITEM_EXPOSURE_TILE)
    tiles_per_block = -(-tiles // min(tiles, _lib.ITEM_EXPOSURE_MAX_BLOCKS))
    per_block = tiles_per_block * _lib.ITEM_EXPOSURE_TILE
    assert per_block > _lib.ITEM_EXPOSURE_BINS and per_block <= n_items        # > slots, and all distinct
    rankings = (torch.arange(entries, dtype=torch.int64, device="cuda") % n_items).to(torch.int32).reshape(U, K)
    # user u holds its own position u % 16 and nothing else
    u = torch.arange(U, dtype=torch.int64, device="cuda")
    truth = ((16 * u + u % 16) % n_items).to(torch.int32)
    gt = ops.CSR(torch.arange(U + 1, dtype=torch.int32, device="cuda"), truth.contiguous())
    w = R.weights(16)
    group_np = (np.arange(n_items) % 5).astype(np.int32)
    e, h, s = raw_exposure(ops, rankings, gt, w, n_items, group_np, 5)
    ids = np.arange(n_items)
    want_e = 4 * w.astype(np.int64)[ids % 16]                            # every item: four entries at position id % 16
    # item i is named by users i // 16 + 2^16 j (j < 4) at position i % 16; user u holds position u % 16
    want_h = np.zeros(n_items, dtype=np.int64)
    for j in range(4):
        holder = ids // 16 + (j << 16)
        want_h += np.where(holder % 16 == ids % 16, w.astype(np.int64)[ids % 16], 0)
    assert np.array_equal(e, want_e) and np.array_equal(h, want_h)
    assert want_h.sum() == sum(int(w[q % 16]) for q in range(16)) * (U // 16)
    want_s = np.stack([np.bincount(group_np, weights=want_e, minlength=5), np.bincount(group_np, weights=want_h, minlength=5)], axis=1)
    assert want_s.max() < 2 ** 53 and np.array_equal(s, want_s.astype(np.int64))      # (float64 weights: exact below 2^53)


def test_unit_weights_equal_item_counts(ops, small):
    rankings, gt, n_items, _ = small
    rs = np.random.RandomState(2)
    cases = [(rankings, gt, 3, n_items), (rankings, gt, 7, n_items)]
    U, n_big = 5000, 70001
    cdf = np.cumsum(1.0 / np.arange(1, n_big + 1))
    zipf = np.minimum(np.searchsorted(cdf / cdf[-1], rs.random_sample((U, 20))), n_big - 1).astype(np.int32)
    cases.append((zipf, [sorted(set(row[rs.random_sample(20) < 0.2].tolist())) for row in zipf], 20, n_big))
    for rk, truth, k, n in cases:
        group_np = rs.randint(0, 6, n).astype(np.int32)
        gt_csr = ops.CSR.from_lists(truth, "cuda")
        rec, hit, sums = ops.item_counts(dev(rk), gt_csr, k, n, dev(group_np), 6)
        e, h, s = raw_exposure(ops, dev(rk), gt_csr, np.ones(k, dtype=np.uint32), n, group_np, 6)
        assert np.array_equal(e, rec.cpu().numpy()) and np.array_equal(h, hit.cpu().numpy())
        assert np.array_equal(s, sums.cpu().numpy()) and e.sum() > 0 and h.sum() > 0


def test_two_calls_return_identical_bytes(ops, small):
    rankings, gt, n_items, _ = small
    group_np = (np.arange(n_items) % 6).astype(np.int32)
    a = raw_exposure(ops, rankings, gt, R.weights(3), n_items, group_np, 6, raw_bytes=True)
    b = raw_exposure(ops, rankings, gt, R.weights(3), n_items, group_np, 6, raw_bytes=True)
    assert a == b
    rk, truth = hot_item(4)
    group_np = (np.arange(60) % 6).astype(np.int32)
    a = raw_exposure(ops, rk, truth, R.weights(4), 60, group_np, 6, raw_bytes=True)
    b = raw_exposure(ops, rk, truth, R.weights(4), 60, group_np, 6, raw_bytes=True)
    assert a == b
