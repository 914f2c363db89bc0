"""The hub-row reduction of the LightGCN SpMM (macr_amd/csrc/spmm_kernels.hip: pieces -> groups of kGroup = 16 -> the row,
summed by whichever wave arrives last; the same code in k_spmm_row and k_spmm_stream) on graphs that reach every branch of
it (tests/spmm_cases.py; tests/test_spmm_plan_cpu.py pins their group counts):

    one group, exactly full / a two-piece hub / a group of ONE piece (no first-level publish) / two groups / more than
    kGroup groups (the second-level loop takes several rounds) -- with and without a plan, pieces in XCD or slot order,
    row kernel and entry stream, half-wave (d = 32) to four columns per lane (d = 256), the batch-row-sparse layers and the
    fused-optimizer finisher of a training step, and the per-process launch switches in fresh child processes.

The propagation tests are EXACT: integer operands scaled by powers of two whose every partial sum is representable in fp32,
so the result must equal an int64 computation bit for bit in any summation order (spmm_cases.exact_case)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spmm_cases as sc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

PLAN_SETTINGS = {                       # None: no plan
    "plan": {},
    "octants0": {"MACR_SPMM_OCTANTS": "0"},
    "noplan": None,
    "stream": {"MACR_SPMM_STREAM": "1"},
    "chunk64": {"MACR_SPMM_CHUNK": "64"},
}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from macr_amd import ops as _ops
    return _ops


_cases, _adj = {}, {}
GRAPHS = {"small": sc.small, "deep": sc.deep, "isolated": sc.isolated, "star": sc.star}


def exact(graph, d, L):
    if (graph, d, L) not in _cases:
        _cases[graph, d, L] = sc.exact_case(GRAPHS[graph](), d, L)
    return _cases[graph, d, L]


def exact_adj(ops, graph, setting):
    """the exact case's matrix (the same for every d and L) on the device, planned under `setting`"""
    if (graph, setting) not in _adj:
        if graph == "deep":
            _adj.clear()                                        # (20 MB plans: keep one graph's at a time)
        _adj[graph, setting] = sc.device_csr(ops, exact(graph, 64, 1)["A"], PLAN_SETTINGS[setting])
    return _adj[graph, setting]


def run_settings(ops, graph, d, L, settings):
    case = exact(graph, d, L)
    print("%s d=%d L=%d: sum|terms| 2^%s, running sum 2^%s granules" % (
        graph, d, L, ["%.1f" % x for x in case["terms_log2"]], ["%.1f" % x for x in case["sums_log2"]]))
    for setting in settings:
        if setting == "stream" and d < 64:
            continue                                            # (d = 32 runs the row kernel)
        adj = exact_adj(ops, graph, setting)
        names = sc.run_exact(ops, case, adj, L, "%s d=%d L=%d %s" % (graph, d, L, setting))
        assert ("spmm_stream" in names) == (setting == "stream"), names


# ----------------------------------------------------------------------------- a. exact propagation
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_hub_rows_propagate_exactly_small(ops, d, L):
    """SMALL under every plan setting.  Row plan: a full single group, groups of one piece, two-piece hubs, two groups per
    row (default: pieces of 1 to 512 entries in XCD order; octants0: slot order; chunk64: up to 10 groups per row and 64
    hub rows); stream: 164 pieces in 13 groups; no plan: one wave per row, 9 000-entry fma chains."""
    run_settings(ops, "small", d, L, ["plan", "octants0", "noplan", "stream", "chunk64"])


@pytest.mark.parametrize("L", [1, 2])
def test_hub_rows_propagate_exactly_deep(ops, L):
    """DEEP: item 0 has 17 groups in the row plan and 33 in the stream -- the second-level loop over more than kGroup groups,
    in both kernels; with 64-entry pieces it has 129 groups (nine rounds)."""
    run_settings(ops, "deep", 64, L, ["plan", "octants0", "noplan", "stream", "chunk64"])


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("d", [64, 128])
def test_rows_without_neighbours_outnumber_the_stream_chunks(ops, d, L):
    """20 000 rows without neighbours beside a graph of a dozen stream chunks: a chunk descriptor names at most 255 of them,
    the rest ride on descriptors without entries.  (Before the plan builder added those, the 8-bit count wrapped and most of
    these rows were never written.)  Every such row is E0 / (L + 1); the output starts as NaN."""
    run_settings(ops, "isolated", d, L, ["plan", "noplan", "stream"])


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_hub_rows_propagate_exactly_star(ops, d, L):
    """STAR: one hub row of 520 entries (two pieces in slot order, eight under the default cuts, nine or sixteen of 64), small
    enough to stay exact through FOUR layers -- the first at which launch_propagate writes a layer into a buffer pair [X | S]
    that an earlier layer wrote (layer 2 reuses pair 0, layer 3 pair 1; three layers never overwrite one)."""
    run_settings(ops, "star", d, L, ["plan", "octants0", "noplan", "stream", "chunk64"])


# ----------------------------------------------------------------------------- b. real weights
@pytest.mark.parametrize("L", [3, 4, 5])
@pytest.mark.parametrize("d", [32, 64])
def test_hub_rows_real_weights_three_layers(ops, d, L):
    """D^-1/2 A D^-1/2 on SMALL, L = 3 and the depths at which layer buffers are reused, 4 and 5 (not exact: guards the rounding
    path) against a float64 product.  Element-wise bound
    L gamma M + 4 u M, u = 2^-24, M = the float64 mean over the layers of |A|^l |E0|, gamma = (chunk + 2 kGroup + number of
    groups of the longest row) u: the first-order worst case of the kernel's summation tree (an fma chain of at most `chunk`
    entries, kGroup partials per group, the groups in rounds of kGroup) per layer, plus the L running-sum additions and the
    final scaling.  Derived, not measured."""
    u = 2.0 ** -24
    A = sc.sym_norm(sc.small())
    rs = np.random.RandomState(5 + d)
    E0 = rs.standard_normal((A.shape[0], d)).astype(np.float32)
    A64, absA = A.astype(np.float64), abs(A).astype(np.float64)
    X, S = E0.astype(np.float64), E0.astype(np.float64)
    Xa, M = np.abs(X), np.abs(X)
    for _ in range(L):
        X = A64 @ X; S = S + X
        Xa = absA @ Xa; M = M + Xa
    want, M = S / (L + 1), M / (L + 1)
    for setting in ("plan", "octants0", "stream"):
        if setting == "stream" and d < 64:
            continue
        adj = sc.device_csr(ops, A, PLAN_SETTINGS[setting])
        P = sc.decode_plan(adj.plan_host)
        tables = P["stream"] if setting == "stream" else P
        n_groups = max(sc.groups_per_row(tables).values())
        assert n_groups >= 2
        gamma = (P["chunk"] + 2 * sc.K_GROUP + n_groups) * u
        bound = L * gamma * M + 4 * u * M
        out = torch.full(E0.shape, float("nan"), dtype=torch.float32, device="cuda")
        got = ops.lgcn_propagate(adj, sc.dev(E0), L, out=out).cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        print("%s d=%d L=%d: max err / bound = %.3g" % (setting, d, L, (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (setting, float((err / np.maximum(bound, 1e-300)).max()))


# ----------------------------------------------------------------------------- c. determinism, counters
@pytest.mark.parametrize("graph", ["small", "deep"])
def test_hub_rows_same_bits_on_every_call_and_counters_return_to_zero(ops, graph):
    """Five propagations on the same plan and the same workspace: all bit-identical (and exact) -- the arrival counters are
    back at zero after every launch and the partial rows are summed in slot order whichever piece finishes last."""
    from macr_amd import _lib
    L, d = 2, 64
    case = exact(graph, d, L)
    N = case["E0"].shape[0]
    for setting in ("plan", "stream"):
        adj = exact_adj(ops, graph, setting)
        ph = adj._plan_ptrs()[1]
        need = _lib.lib().macr_lgcn_work_floats(N, d, ph)
        work = torch.zeros(need, dtype=torch.float32, device="cuda")
        outs = []
        for k in range(5):
            out = torch.empty((N, d), dtype=torch.float32, device="cuda")
            sc.run_exact(ops, case, adj, L, "%s %s call %d" % (graph, setting, k), work=work, out=out)
            outs.append(out)
        for k in range(1, 5):
            assert torch.equal(outs[0].view(torch.int32), outs[k].view(torch.int32)), (setting, k)
        # the arrival counters sit behind the layer buffers and the slab of partial rows (macr_lgcn_work_floats)
        P = sc.decode_plan(adj.plan_host)
        S = P["stream"] or P
        slab_rows = max(P["n_slots"] + P["n_groups"], S["n_slots"] + S["n_groups"])
        counters = work[4 * N * d + slab_rows * d:].view(torch.int32)
        assert counters.numel() >= max(P["n_groups"] + P["n_split"], S["n_groups"] + S["n_split"])
        assert not counters.any()


# ----------------------------------------------------------------------------- d. training step
def _kinds(ops):
    return [ops.LOSS_NORMALBCE, ops.LOSS_RUBIBCEBOTH, ops.LOSS_BPR_LGCN]


@pytest.mark.parametrize("kind_name", ["LOSS_NORMALBCE", "LOSS_RUBIBCEBOTH", "LOSS_BPR_LGCN"])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_train_step_with_multi_group_hub_rows(ops, d, kind_name):
    """SMALL, L = 2, B = 256, three steps (spmm_cases.run_train_case): the batch-row-sparse last forward layer leaves the hub
    rows to their pieces, the first backward layer gathers row-sparse input through two-group hub rows (d = 32, 128) or runs
    dense (d = 64), and the finisher of a hub row applies the fused optimizer with reference counts >= 3 (item 0), 1 (item 4)
    and 0 (item 2)."""
    sc.run_train_case(ops, d, getattr(ops, kind_name), {})


def test_train_step_with_hub_rows_in_both_plans(ops):
    """the row-normalised adjacency D^-1 A forward and its transpose backward: multi-group hub rows in both plans"""
    sc.run_train_case(ops, 64, ops.LOSS_RUBIBCEBOTH, {}, asym=True)


# ----------------------------------------------------------------------------- e. per-process switches
CHILDREN = [
    ("stream_fused", {"MACR_SPMM_STREAM": "1", "MACR_SPMM_STREAM_FUSED": "1"}),
    ("records0", {"MACR_SPMM_RECORDS": "0"}),
    ("bwd1_sparse", {"MACR_LGCN_BWD1_DENSE": "0"}),
    ("bwd1_dense", {"MACR_LGCN_BWD1_DENSE": "1"}),
]
_child_failed = []


@pytest.mark.parametrize("name,env", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_launch_switches_in_a_fresh_process(ops, name, env):
    """MACR_SPMM_STREAM_FUSED, MACR_SPMM_RECORDS and MACR_LGCN_BWD1_DENSE are latched by the first launch of a process, so each
    setting runs tests/spmm_knob_worker.py in a child of its own: the exact SMALL d = 64 propagation and a training case,
    with the kernel names the setting must select.  One child at a time; this process launches nothing while it runs; after
    a child that failed or ran out of time no further child is started."""
    if _child_failed:
        pytest.fail("not started: the child for %s failed" % _child_failed[0])
    torch.cuda.synchronize()
    child_env = {k: v for k, v in os.environ.items() if not k.startswith(("MACR_SPMM_", "MACR_LGCN_"))}
    child_env.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "spmm_knob_worker.py"), name], env=child_env, timeout=120,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    except subprocess.TimeoutExpired:
        _child_failed.append(name)
        raise
    if r.returncode != 0:
        _child_failed.append(name)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    verdict = json.loads(r.stdout.strip().splitlines()[-1])
    print(verdict)
    assert verdict["ok"] and verdict["setting"] == name, verdict
