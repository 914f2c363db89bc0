"""The radix sort of the row references (macr_amd/csrc/refsort.hpp::launch_radix_sort) against numpy, pair by pair (-m gpu).

Every training step above 8192 triples, and every deterministic and row-sharded step, sums a gradient row over the run the sort
puts its references in; whole steps compared with a tolerance do not notice one misplaced pair.  Here the sort runs alone
(macr_test_radix_sort, libmacr_hip_test.so) and must equal np.argsort(keys, kind="stable") exactly: keys AND values, the values
an arbitrary permutation so that a swapped pairing shows.  Covered: sizes around the wave (64), the sort batch (512), the three
tile sizes (2048 / 8192 / 16384 keys, the last one only above 2^20 pairs -- no training test is that large) and the tile
thresholds 2^17 and 2^20; 1, 2, 3 and 4 passes (max_key of 8 .. 32 bits); keys all equal, descending, varying in the top or the
low byte only, Zipf and uniform.  Each size runs once with a law and a pass count that rotate, the full pass x law grid at one
small and one mid size, and every size again under each forced MACR_SORT_TILE in a child process of its own
(tests/refsort_worker.py; the knob is latched per process): 2^20 + 1 pairs in 513 tiles of 2048, 65 pairs in one tile of 16384."""
import json
import os
import subprocess
import sys

import pytest
import torch

import refsort_worker as rw

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    assert not os.environ.get("MACR_SORT_TILE"), "the in-process sorts take the default tile"
    from macr_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("n,law,bits", rw.rotation(), ids=["n%d-%s-%dbit" % c for c in rw.rotation()])
def test_sort_is_numpys_stable_sort(ops, n, law, bits):
    assert ops.test_sort_tile_for(n) == rw.default_tile(n)          # n = 2^20 + 1: the 16384-key kernels
    rw.check_sort(ops, n, law, bits)


def test_every_size_law_and_pass_count_is_in_the_rotation():
    rot = rw.rotation()
    assert [n for n, _, _ in rot] == list(rw.NS) and set(l for _, l, _ in rot) == set(rw.LAWS) and set(b for _, _, b in rot) == set(rw.BITS)
    assert sorted(set(rw.passes_of(b) for b in rw.BITS)) == [1, 2, 3, 4]
    assert rw.default_tile(rw.NS[-1]) == 16384 and rw.passes_of(rot[-1][2]) == 4


@pytest.mark.parametrize("n", [513, 16385])
def test_every_pass_count_with_every_key_law(ops, n):
    """513: one partial tile, nine 64-key rounds of which the last holds one key; 16385: nine tiles of 2048, the last with one key"""
    for bits in rw.BITS:
        for law in rw.LAWS:
            rw.check_sort(ops, n, law, bits)


_child_failed = []


@pytest.mark.parametrize("tile", rw.TILES)
def test_every_size_under_a_forced_tile(ops, tile):
    """MACR_SORT_TILE = 2048, 8192, 16384: the rotation again, every size at that tile.  One child process per value, one at a
    time; after a child that failed or ran out of time no further child is started."""
    if _child_failed:
        pytest.fail("not started: the child for tile %d failed" % _child_failed[0])
    torch.cuda.synchronize()
    env = dict(os.environ, MACR_SORT_TILE=str(tile))
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "refsort_worker.py"), "sort"], env=env, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    except subprocess.TimeoutExpired:
        _child_failed.append(tile)
        raise
    if r.returncode != 0:
        _child_failed.append(tile)
    assert r.returncode == 0, (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    assert verdict["ok"] and verdict["tile"] == tile, verdict
    assert [tuple(x) for x in verdict["done"]] == rw.rotation()
