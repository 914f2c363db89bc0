"""NumPy restatement of the full-catalogue position of a (query, item) pair, shared by tests/test_rank_positions_cpu.py and
tests/test_gpu_rank_positions.py: the project's (score, id) key (common.hpp::make_key) as 64-bit integers, and plain
integer counting over a row of scores."""
import numpy as np


def keys(scores_row):
    """uint64[N]: larger = ranks earlier (score descending, id ascending, -0.0 ties with +0.0); 0 for a NaN score"""
    s = np.ascontiguousarray(scores_row, dtype=np.float32)
    u = s.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    o = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    k = (o << np.uint64(32)) | (np.uint64(0xffffffff) - np.arange(len(s), dtype=np.uint64))
    k[np.isnan(s)] = 0
    return k


def positions(scores, mask_lists, pair_lists):
    """int32[n_pairs] in CSR order: candidates of the query (items outside its mask) whose key is larger than the pair's;
    -1 for a pair that is masked, outside [0, N) or NaN.  scores float32 (U, N)."""
    U, N = scores.shape
    out = []
    for q in range(U):
        k = keys(scores[q])
        cand = np.ones(N, dtype=bool)
        m = np.asarray([i for i in mask_lists[q] if 0 <= i < N], dtype=np.int64)
        cand[m] = False
        ck = k[cand]
        for g in pair_lists[q]:
            if g < 0 or g >= N or not cand[g] or np.isnan(scores[q, g]):
                out.append(-1)
            else:
                out.append(int((ck > k[g]).sum()))
    return np.asarray(out, dtype=np.int32)


def pair_scores(scores, pair_lists):
    """float32[n_pairs] in CSR order; NaN for an item outside [0, N)"""
    N = scores.shape[1]
    return np.asarray([scores[q, g] if 0 <= g < N else np.nan for q in range(len(pair_lists)) for g in pair_lists[q]],
                      dtype=np.float32)
