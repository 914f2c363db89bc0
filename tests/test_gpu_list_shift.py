"""macr_list_shift (the kernel behind MACR_SHIFT_REPORT) on the GPU against the plain-loop restatement (tests/shift_ref.py):
every output array bit for bit, on output buffers pre-filled with garbage.  Shapes: the smallest at which the kernel can go
wrong -- k = 1, one query, unequal row strides, k at and past one entry per lane (64, 65, 128), query counts that are no
multiple of the four queries of a workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import item_acc_ref
import shift_ref as R

pytestmark = pytest.mark.gpu

GARBAGE = 0x5a
N_ITEMS = 1000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dirty(*shape):
    return torch.full(shape, GARBAGE, dtype=torch.uint8, device="cuda").view(torch.int32)


def raw_shift(ops, base, here, gt, k, n_items, U=None, K_base=None, K_here=None, null=None):
    """macr_list_shift through the C ABI on garbage-filled outputs -> (return code, per_user, entered, left as NumPy int32)"""
    from macr_amd import _lib
    rows = base.shape[0]
    tens = {"rank_base": dev(base.astype(np.int32)), "rank_here": dev(here.astype(np.int32)),
            "gt_ptr": gt.ptr, "gt_idx": gt.idx,
            "per_user": dirty(rows, 32), "entered": dirty(rows, 4 * max(k, 1)), "left": dirty(rows, 4 * max(k, 1))}
    p = lambda name: None if name == null else ctypes.c_void_p(tens[name].data_ptr())
    rc = _lib.lib().macr_list_shift(rows if U is None else U, base.shape[1] if K_base is None else K_base,
                                    here.shape[1] if K_here is None else K_here, k, p("rank_base"), p("rank_here"), p("gt_ptr"),
                                    p("gt_idx"), n_items, p("per_user"), p("entered"), p("left"),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, tens["per_user"].cpu().numpy(), tens["entered"].cpu().numpy(), tens["left"].cpu().numpy()


def make_case(seed, U, K_base, K_here, k, n_items=N_ITEMS):
    """Two rankings and ground-truth lists.  Random rows: full or with -1 tails of different lengths, any share of common ids
    in any order; the slots past k (up to the strides) hold ids of the OTHER row, which the call must not read.  With
    U >= 5 the first rows are: identical; disjoint; the same set reversed; an empty base row; -1 in the middle, ids >= n_items
    and 2^31 - 1.  Every fourth query has an empty ground truth, the others hold kept, gained and lost ids and strangers."""
    rs = np.random.RandomState(seed)
    base = np.full((U, K_base), -1, dtype=np.int32)
    here = np.full((U, K_here), -1, dtype=np.int32)
    gt = []
    for u in range(U):
        pool = rs.permutation(n_items).astype(np.int32)
        nb = k if rs.rand() < 0.5 else rs.randint(0, k + 1)
        nh = k if rs.rand() < 0.5 else rs.randint(0, k + 1)
        share = rs.randint(0, min(nb, nh) + 1)
        b = pool[:nb]
        h = np.concatenate([rs.permutation(b)[:share], pool[nb:nb + nh - share]])
        rs.shuffle(h)
        if U >= 5 and u == 0:
            h = b.copy()
        elif U >= 5 and u == 1:
            b, h = pool[:k], pool[k:2 * k]
        elif U >= 5 and u == 2:
            b = pool[:k]
            h = b[::-1].copy()
        elif U >= 5 and u == 3:
            b, h = pool[:0], pool[:k]
        elif U >= 5 and u == 4:
            b, h = pool[:k].copy(), rs.permutation(pool[:k])
            b[0], h[0] = n_items, n_items + 3
            if k >= 3:
                b[k // 2], h[k // 3] = -1, -1
                b[k - 1] = 2 ** 31 - 1
        base[u, :len(b)], here[u, :len(h)] = b, h
        base[u, k:] = np.resize(np.concatenate([h, pool[-3:]]), K_base - k)        # never read
        here[u, k:] = np.resize(np.concatenate([b, pool[-3:]]), K_here - k)
        if u % 4 == 0:
            gt.append([])
            continue
        vb, vh = (set(int(x) for x in r if 0 <= x < n_items) for r in (b, h))
        pick = lambda s: [x for x in sorted(s) if rs.rand() < 0.3]
        gt.append(sorted(set(pick(vb & vh) + pick(vh - vb) + pick(vb - vh) + rs.randint(0, n_items, 3).tolist())))
    return base, here, gt


SHAPES = [(1, 1, 1, 1), (5, 1, 4, 1), (1, 20, 20, 20), (5, 20, 20, 20), (5, 20, 32, 20), (259, 32, 20, 20), (5, 64, 64, 64),
          (6, 128, 65, 65), (5, 128, 128, 128), (259, 128, 128, 128)]


@pytest.mark.parametrize("U,K_base,K_here,k", SHAPES)
def test_every_output_bit_for_bit(ops, U, K_base, K_here, k):
    base, here, gt = make_case(100 * U + k, U, K_base, K_here, k)
    want = R.list_shift(base, here, gt, k, N_ITEMS)
    csr = ops.CSR.from_lists(gt, "cuda")
    rc, pu, ent, left = raw_shift(ops, base, here, csr, k, N_ITEMS)
    assert rc == 0
    for got, ref, name in zip((pu, ent, left), want, ("per_user", "entered", "left")):
        assert got.dtype == np.int32 and got.shape == ref.shape and got.tobytes() == ref.tobytes(), (name, np.argwhere(got != ref)[:5])
    again = raw_shift(ops, base, here, csr, k, N_ITEMS)                    # two calls, the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], (pu, ent, left)))
    # the torch face
    t = ops.list_shift(dev(base), dev(here), csr, k, N_ITEMS)
    assert all(x.dtype == torch.int32 for x in t) and t[0].shape == (U, 8) and t[1].shape == t[2].shape == (U, k)
    assert all(np.array_equal(x.cpu().numpy(), ref) for x, ref in zip(t, want))
    if U >= 5:                                                             # the hand-made rows are what they claim
        assert pu[0, 3] == k and pu[0, 2] == pu[0, 1] and (ent[0] == -1).all()                  # identical
        assert pu[1, 2] == 0 and (ent[1] >= 0).all() and (left[1] >= 0).all()                   # disjoint
        assert pu[2, 2] == k and (ent[2] == -1).all() and (pu[2, 4] > 0 or k == 1)              # reversed: footrule > 0
        assert pu[3, 0] == 0 and pu[3, 1] == k and (left[3] == -1).all()                        # empty base row
        assert pu[4, 0] < k and pu[4, 3] == 0                                                   # skipped slots
    if U >= 200:
        assert (pu[:, 7] > 0).any() and (pu[:, 6] > pu[:, 7]).any() and (pu[:, 5] > pu[:, 7]).any()     # kept, gained, lost hits


def test_entered_feeds_item_counts_and_rank_pairs(ops):
    """`entered` is a `rankings` of macr_item_counts: per item how often it entered a list, and how often as a gained hit"""
    U, k = 259, 20
    base, here, gt = make_case(7, U, 32, 20, k)
    _, want_ent, want_left = R.list_shift(base, here, gt, k, N_ITEMS)
    csr = ops.CSR.from_lists(gt, "cuda")
    _, ent, left = ops.list_shift(dev(base), dev(here), csr, k, N_ITEMS)
    group_np = (np.arange(N_ITEMS) % 6).astype(np.int32)
    for got, ref in ((ent, want_ent), (left, want_left)):
        rec, hit, sums = ops.item_counts(got, csr, k, N_ITEMS, dev(group_np), 6)
        want_rec = np.zeros(N_ITEMS, dtype=np.int64)
        want_hit = np.zeros(N_ITEMS, dtype=np.int64)
        for u in range(U):
            for i in ref[u]:
                if i >= 0:
                    want_rec[i] += 1
                    want_hit[i] += int(i in gt[u])
        assert want_hit.any()
        assert np.array_equal(rec.cpu().numpy(), want_rec) and np.array_equal(hit.cpu().numpy(), want_hit)
        assert np.array_equal(sums.cpu().numpy(), item_acc_ref.group_sums(group_np, want_rec, want_hit, 6))
    # ascending within a row: the non-negative entries are a pair list as macr_rank_positions takes it
    e = ent.cpu().numpy()
    for row in e:
        ids = row[row >= 0]
        assert (np.diff(ids) > 0).all() and (row[len(ids):] == -1).all()


def test_every_refusal_leaves_the_outputs_untouched(ops):
    from macr_amd import _lib
    base, here, gt = make_case(3, 5, 32, 20, 20)
    csr = ops.CSR.from_lists(gt, "cuda")
    wide = np.full((5, 129), -1, dtype=np.int32)
    cases = [dict(U=0), dict(U=-1), dict(k=0), dict(k=-3), dict(k=21), dict(k=33), dict(n_items=0), dict(n_items=-1),
             dict(base=wide, k=20), dict(here=wide, k=20), dict(K_base=129), dict(K_here=129)]
    cases += [dict(null=name) for name in ("rank_base", "rank_here", "gt_ptr", "gt_idx", "per_user", "entered", "left")]
    for case in cases:
        kw = dict(case)
        rc, pu, ent, left = raw_shift(ops, kw.pop("base", base), kw.pop("here", here), csr, kw.pop("k", 20),
                                      kw.pop("n_items", N_ITEMS), **kw)
        assert rc == _lib.E_INVALID and b"list_shift" in _lib.lib().macr_last_error(), case
        for out in (pu, ent, left):
            assert (out.view(np.uint8) == GARBAGE).all(), case
    with pytest.raises(ops.MacrError):
        ops.list_shift(dev(base), dev(here[:4]), csr, 20, N_ITEMS)
    with pytest.raises(ops.MacrError):
        ops.list_shift(dev(base), dev(here), csr, 21, N_ITEMS)
