"""The staged gradient path -- reference keys, the sort, and the four row reductions behind it -- against exact integer sums, bit
for bit (-m gpu).

tests/seg_cases.py prescribes where every run of the sorted reference list lies and fills the staging rows with integers in
[-7, 7], so that fp32 addition is exact in any order (max over rows of sum |terms| < 2^24, asserted by
tests/test_seg_cases_cpu.py together with the presence of every feature a case is named for).  macr_test_ref_reduce
(libmacr_hip_test.so) runs the product's own launchers on such a batch: k_refs_init for whole tables, k_shard_keys under an
ownership description, launch_radix_sort, then per mode
    reduce   k_seg_reduce                      (atomics for runs cut into chunks)
    index    k_seg_scan + k_seg_sum            (flags (len << 26) | position for runs of <= 16, work items beyond)
    det      k_seg_reduce<., true> + k_seg_fold
    inv      k_seg_reduce_inv + k_seg_fold_inv (through k_shard_keys in every case)
No tolerance: the sorted list equals the stable sort of the keys, every referenced row equals its int64 sum, every other word of
the outputs -- unreferenced rows, the rows behind each table where a foreign key taken for a row would land, their flags -- is
what it was.  Rows a mode stores start as NaN, rows it adds to atomically as zero: a row nobody wrote, or one written by the
other route, cannot pass.  Each call is repeated on the same workspace with fresh outputs (the work counter and the sort's digit
totals are re-armed by the call itself).

A mismatch names the table, row and column and prints the run's layout() record: its heads, slots, chunk counts and work items
say which piece of index arithmetic owns the lost or doubled reference."""
import os

import pytest
import torch

import seg_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    assert not os.environ.get("MACR_SORT_TILE"), "the cases sort at the default tile"
    from macr_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("d,name", sc.CASE_IDS, ids=["d%d-%s" % c for c in sc.CASE_IDS])
def test_row_sums_equal_the_integer_model(ops, d, name):
    c = sc.case(d, name)
    inputs = sc.upload(c)
    for mode in sc.MODES:
        got, ws = sc.run_on_gpu(ops, c, mode, inputs)
        sc.compare(c, mode, got)
        again, _ = sc.run_on_gpu(ops, c, mode, inputs, ws)          # the same workspace, outputs reset
        sc.compare(c, mode, again)


def test_a_lost_reference_cannot_pass():
    """host only: the comparison above fails against a model that lost one reference of a 16 040-reference row"""
    assert sc.sensitivity_check() >= 6700
