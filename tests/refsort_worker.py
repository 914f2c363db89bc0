"""Cases of tests/test_gpu_refsort.py and the workspace rule of tests/test_seg_cases_cpu.py, importable and runnable as a worker.

MACR_SORT_TILE (refsort.hpp::sort_tile_for) is latched in a static by the first sort of a process, so every forced tile gets a
process of its own with the knob in its environment:

    MACR_SORT_TILE=2048 python tests/refsort_worker.py sort     the sizes of NS under that tile, on the GPU
    MACR_SORT_TILE=2048 python tests/refsort_worker.py hist     the workspace rule under that tile, host only

Both print one JSON verdict line.  The reference of a sort is numpy: np.argsort(keys, kind="stable")."""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

NS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 16385, 1 << 17, (1 << 17) + 1, 1 << 20, (1 << 20) + 1)
BITS = (8, 9, 16, 17, 24, 25, 32)                 # max_key = 2^bits - 1: 1, 2, 2, 3, 3, 4 and 4 passes of 8 bits
LAWS = ("equal", "descending", "top_byte", "low_byte", "zipf", "uniform")
TILES = (2048, 8192, 16384)


def passes_of(bits):
    return (bits + 7) // 8


def default_tile(n):
    return 2048 if n <= 1 << 17 else 8192 if n <= 1 << 20 else 16384


def make_pairs(law, n, bits, seed=0):
    """-> keys, vals (uint32[n]), max_key.  Values: a permutation of 0 .. n-1 that is not the identity."""
    rng = np.random.RandomState((seed + 7919 * n + 31 * bits + LAWS.index(law)) % (1 << 32))
    max_key = (1 << bits) - 1
    if law == "equal":                            # pure stability: the values must come back in their order
        keys = np.full(n, max_key, np.uint64)
    elif law == "descending":                     # strictly descending where 2^bits keys allow it, else non-increasing
        k = np.arange(n, dtype=np.uint64)
        keys = max_key - k if n <= max_key + 1 else ((n - 1 - k) << np.uint64(bits)) // np.uint64(n)
    elif law == "top_byte":                       # only the last pass's digit varies (the top 8 of `bits`)
        keys = (rng.randint(0, 256, n).astype(np.uint64) << np.uint64(bits - 8)) | np.uint64(0x5A5A5A & ((1 << (bits - 8)) - 1))
    elif law == "low_byte":                       # only the first pass's digit varies
        keys = np.uint64(max_key & ~0xFF) | rng.randint(0, 256, n).astype(np.uint64)
    elif law == "zipf":
        keys = np.minimum(rng.zipf(1.3, n).astype(np.uint64) - 1, max_key)
    else:
        keys = rng.randint(0, 1 << 32, n, dtype=np.uint64) & np.uint64(max_key)
    assert keys.max() <= max_key
    vals = rng.permutation(n).astype(np.uint32)
    if n > 2:
        assert not np.array_equal(vals, np.arange(n))
    return keys.astype(np.uint32), vals, max_key


def rotation():
    """each n once, with a law and a pass count that rotate"""
    return [(n, LAWS[(k + 3) % len(LAWS)], BITS[(2 * k + 5) % len(BITS)]) for k, n in enumerate(NS)]


def check_sort(ops, n, law, bits, device="cuda"):
    """one sort on the GPU against numpy; raises AssertionError"""
    import torch
    keys, vals, max_key = make_pairs(law, n, bits)
    order = np.argsort(keys, kind="stable")
    dk, dv = (torch.from_numpy(a.view(np.int32)).to(device) for a in (keys, vals))
    ko, vo = ops.test_radix_sort(dk, dv, max_key)
    torch.cuda.synchronize()
    ko, vo = ko.cpu().numpy().view(np.uint32), vo.cpu().numpy().view(np.uint32)
    what = "n=%d %s %d bits (%d passes, tile %d)" % (n, law, bits, passes_of(bits), ops.test_sort_tile_for(n))
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), keys), what + ": the input keys were changed"
    assert np.array_equal(ko, np.sort(keys)), what + ": keys not sorted; first at %d" % int(np.flatnonzero(ko != np.sort(keys))[0])
    assert np.array_equal(ko, keys[order])
    bad = np.flatnonzero(vo != vals[order])
    assert len(bad) == 0, what + ": %d values differ from the stable order, first at %d (key 0x%x)" % (len(bad), int(bad[0]), int(ko[bad[0]]))


def hist_need(ops, n):
    """words one sort of n pairs touches: a row of 256 counts per tile + the digit totals of 4 passes"""
    tile = ops.test_sort_tile_for(n)
    return 256 * ((n + tile - 1) // tile) + 4 * 256


def hist_sweep():
    ns = set([1, 2, 100, 3 << 20, (3 << 20) + 5, 1 << 22])
    for e in (2048, 8192, 16384, 1 << 17, 1 << 20):
        ns.update([e - 1, e, e + 1, 2 * e - 1, 2 * e + 1])
    rng = np.random.RandomState(5)
    ns.update(int(x) for x in rng.randint(1, 3 << 20, 200))
    return sorted(ns)


def check_hist_rule(ops, forced=None):
    """sort_hist_words(n) is non-decreasing and covers every sort of up to n pairs at the tile that sort takes"""
    prev, need_max = 0, 0
    for n in hist_sweep():
        tile = ops.test_sort_tile_for(n)
        assert tile == (forced or default_tile(n)), (n, tile, forced)
        words = ops.test_sort_hist_words(n)
        need_max = max(need_max, hist_need(ops, n))
        assert words >= prev, "sort_hist_words decreases at n=%d: %d < %d" % (n, words, prev)
        assert words >= need_max, "sort_hist_words(%d) = %d < %d words a sort of at most that many pairs writes" % (n, words, need_max)
        prev = words
    return len(hist_sweep())


def main(what):
    sys.path.insert(0, os.path.dirname(HERE))
    forced = int(os.environ["MACR_SORT_TILE"]) if os.environ.get("MACR_SORT_TILE") else None
    res = {"what": what, "tile": forced, "ok": False, "done": []}
    from macr_amd import ops
    try:
        if what == "hist":
            res["done"] = check_hist_rule(ops, forced)
        else:
            for n, law, bits in rotation():
                assert ops.test_sort_tile_for(n) == (forced or default_tile(n))
                check_sort(ops, n, law, bits)
                res["done"].append([n, law, bits])
        res["ok"] = True
    except AssertionError:
        res["error"] = traceback.format_exc()[-3000:]
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
