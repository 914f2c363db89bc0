"""The native reference-stream sampler (macr_ref_sample_batches, macr_amd/host_sampler.py) against the Python form it
replaces -- MFData.sample, LGCNData.sample, LGCNData.sample_test -- and against the goldens captured from the reference
(G2 / G3): the same batches and the same `random` / `numpy.random` states, bit for bit.  No GPU anywhere."""
import collections
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLD, REPO, dataset_args, golden
from macr_amd import _lib
from macr_amd.build import build
from macr_amd.data import LGCNData, MFData
from macr_amd.host_sampler import ReferenceStreamSampler


@pytest.fixture(scope="module", autouse=True)
def _built():
    build()


# ---- the live generator states ----------------------------------------------------------------------------------------
def seed_all(seed, mid_block=False):
    """seed both modules; mid_block: also move both generators off the block boundary (position != 624) and fill numpy's
    Gaussian cache, which a pass must carry through untouched"""
    random.seed(seed)
    np.random.seed(seed)
    if mid_block:
        for _ in range(5):
            random.random()
        random.gauss(0.0, 1.0)
        np.random.randint(0, 1000, size=7)
        np.random.standard_normal(1)
        assert random.getstate()[1][624] not in (0, 624) and np.random.get_state()[2] not in (0, 624)
        assert np.random.get_state()[3] == 1 and random.getstate()[2] is not None


def states():
    ver, internal, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return (ver, internal, gauss), (kind, keys.tobytes(), int(pos), int(has_gauss), float(cached))


def python_form(fn, n):
    return np.asarray([fn() for _ in range(n)], dtype=np.int32).reshape(n, 3, -1)


# ---- datasets -----------------------------------------------------------------------------------------------------------
_DATA = {}


def mf_data(name):
    if ("mf", name) not in _DATA:
        _DATA["mf", name] = MFData(dataset_args(name))
    return _DATA["mf", name]


def lgcn_data(name):
    if ("lgcn", name) not in _DATA:
        a = dataset_args(name)
        _DATA["lgcn", name] = LGCNData(path=a.data_path + a.dataset, batch_size=a.batch_size, args=a)
    return _DATA["lgcn", name]


def synth_mf(lists, n_users, n_items, B):
    """an MFData with exactly the fields sample() reads (no files)"""
    d = object.__new__(MFData)
    d.n_users, d.n_items, d.batch_size = n_users, n_items, B
    d.users, d.items = list(range(n_users)), list(range(n_items))
    d.train_user_list = collections.defaultdict(list)
    d.train_user_list.update({u: list(v) for u, v in lists.items() if len(v)})
    d._train_sets = {}
    return d


def synth_lgcn(lists, exist_users, n_users, n_items, B, test_lists=None):
    """an LGCNData with exactly the fields sample() / sample_test() read (no files)"""
    d = object.__new__(LGCNData)
    d.n_users, d.n_items, d.batch_size = n_users, n_items, B
    d.exist_users = list(exist_users)
    d.train_items = {u: list(v) for u, v in lists.items() if len(v)}
    d.test_set = {u: list(v) for u, v in (test_lists or {}).items()}
    d._train_sets = {}
    return d


def check_equal(sampler, fn, n, seed=12345, mid_block=True, passes=None):
    """n batches: the Python form from `seed`, then the native form from the same seed (in the given passes); batches and
    final states must agree"""
    seed_all(seed, mid_block)
    want = python_form(fn, n)
    after = states()
    seed_all(seed, mid_block)
    got = np.concatenate([sampler.generate(m) for m in (passes or [n])])
    assert np.array_equal(got, want)
    assert states() == after
    return want


# ---- goldens captured from the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["addressa", "tiny"])
def test_golden_g2_mf_stream_through_the_native_path(name):
    want = np.load(os.path.join(GOLD, "G2_mf_sampler_%s.npz" % name))["batches"]
    seed = golden("mf", name)["G2"]["seed"]
    random.seed(seed)
    np.random.seed(seed)
    got = ReferenceStreamSampler.for_mf(mf_data(name)).generate(want.shape[0])
    assert got.dtype == np.int32 and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["addressa", "tiny"])
def test_golden_g3_lgcn_streams_through_the_native_path(name):
    z = np.load(os.path.join(GOLD, "G3_lgcn_sampler_%s.npz" % name))
    seed = golden("lgcn", name)["G3"]["seed"]
    assert "sample_test" in z.files
    for key, test in (("sample", False), ("sample_test", True)):
        random.seed(seed)
        np.random.seed(seed)
        got = ReferenceStreamSampler.for_lgcn(lgcn_data(name), test=test).generate(z[key].shape[0])
        assert np.array_equal(got, z[key]), key


# ---- long runs against the live modules --------------------------------------------------------------------------------
PASS, LONG = 111, 1000


@pytest.mark.parametrize("stream", ["mf", "lgcn"])
def test_thousand_addressa_batches_in_passes_and_hand_over_both_ways(stream):
    """1000 consecutive batches natively in passes of 111 = the Python form; the live states agree after EVERY pass; then
    three Python-form batches after the native passes, and a native pass after those, continue the all-Python run."""
    if stream == "mf":
        data = mf_data("addressa")
        fn, sampler = data.sample, ReferenceStreamSampler.for_mf(data)
    else:
        data = lgcn_data("addressa")
        fn, sampler = data.sample, ReferenceStreamSampler.for_lgcn(data)
    bounds = list(range(PASS, LONG, PASS)) + [LONG]                     # ends of the native passes
    total = LONG + 3 + PASS
    seed_all(2024)
    want, at = [], {}
    for k in range(total):
        want.append(fn())
        at[k + 1] = states() if (k + 1) in bounds or k + 1 in (LONG + 3, total) else None
    want = np.asarray(want, dtype=np.int32)

    seed_all(2024)
    lo = 0
    for hi in bounds:
        got = sampler.generate(hi - lo)
        assert np.array_equal(got, want[lo:hi]), (lo, hi)
        assert states() == at[hi], "states after the pass ending at batch %d" % hi
        lo = hi
    mid = python_form(fn, 3)                                             # Python form after a native pass
    assert np.array_equal(mid, want[LONG:LONG + 3]) and states() == at[LONG + 3]
    got = sampler.generate(PASS)                                         # native pass after Python-form batches
    assert np.array_equal(got, want[LONG + 3:]) and states() == at[total]


def test_lgcn_sample_test_pass_follows_a_native_training_pass_and_the_reverse():
    data = lgcn_data("addressa")
    train, test = ReferenceStreamSampler.for_lgcn(data), ReferenceStreamSampler.for_lgcn(data, test=True)
    seed_all(77, mid_block=True)
    want = [python_form(data.sample, 4), python_form(data.sample_test, 4), python_form(data.sample, 4),
            python_form(data.sample_test, 3)]
    after = states()
    seed_all(77, mid_block=True)
    got = [train.generate(4), python_form(data.sample_test, 4), python_form(data.sample, 4), test.generate(3)]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert states() == after


# ---- chunking -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["mf", "lgcn", "lgcn_test"])
@pytest.mark.parametrize("mid_block", [False, True])
def test_chunking_changes_neither_batches_nor_states(stream, mid_block):
    """chunks of 1, 7 and the whole pass; the pass spans many twists (40 batches of 1024 triples draw > 120 000 words of
    a 624-word block) and starts on a block boundary or in the middle of a block"""
    n = 40
    if stream == "mf":
        data = mf_data("addressa")
        fn, make = data.sample, lambda c: ReferenceStreamSampler.for_mf(data, chunk_batches=c)
    else:
        data = lgcn_data("addressa")
        fn = data.sample_test if stream == "lgcn_test" else data.sample
        make = lambda c: ReferenceStreamSampler.for_lgcn(data, test=stream == "lgcn_test", chunk_batches=c)
    seed_all(5, mid_block)
    want = python_form(fn, n)
    after = states()
    for chunk in (1, 7, n):
        seed_all(5, mid_block)
        s = make(chunk)
        s.begin_pass(n)                                                   # (device=None: host tensors)
        got = np.stack([s.sample().numpy() for _ in range(n)])
        assert np.array_equal(got, want), chunk
        assert states() == after, chunk
    with pytest.raises(RuntimeError):
        s.sample()                                                        # a pass hands out n batches, no more


# ---- edge cases on small synthetic data --------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257)


def edge_lists(n_users, n_items, rs, with_empty):
    """user k < 8: an unsorted list of LENGTHS[k] items with a repeated one; user 8: empty (with_empty) ; user 9: the whole
    catalogue minus one item; the rest: short random lists.  Items stay below n_items - 1, so no list covers the catalogue."""
    lists = {}
    for u in range(n_users):
        if u < len(LENGTHS):
            v = rs.randint(0, n_items - 1, size=LENGTHS[u]).tolist()
            if len(v) > 1:
                v[-1] = v[0]
        elif u == 8:
            v = [] if with_empty else [0]
        elif u == 9:
            v = [x for x in rs.permutation(n_items).tolist() if x != n_items // 2]
        else:
            v = rs.randint(0, n_items - 1, size=1 + u % 6).tolist()
        lists[u] = v
    return lists


@pytest.mark.parametrize("n_items", [2, 256, 257, 744])
def test_edge_lists_and_catalogue_sizes(n_items):
    """positive lists of length 1..257 (1 draws no word under NumPy and at least one under Python), unsorted with a repeat;
    an empty list under MF (item 0, no draw); an exclusion list of the catalogue minus one item; n_items around powers of 2"""
    rs = np.random.RandomState(n_items)
    n_users, B = 24, 16
    lists = edge_lists(n_users, n_items, rs, with_empty=True)
    d = synth_mf(lists, n_users, n_items, B)
    want = check_equal(ReferenceStreamSampler.for_mf(d), d.sample, 30, seed=n_items)
    hit = want[:, 0, :] == 8
    assert hit.any() and (want[:, 1, :][hit] == 0).all()                 # the empty list gives item 0
    hit = want[:, 0, :] == 9
    assert hit.any() and (want[:, 2, :][hit] == n_items // 2).all()      # the only item left
    lists = edge_lists(n_users, n_items, rs, with_empty=False)
    tests = {u: rs.randint(0, n_items - 1, size=1 + u % 3).tolist() for u in range(0, n_users, 2) if u != 9}
    g = synth_lgcn(lists, range(n_users), n_users, n_items, B, tests)
    check_equal(ReferenceStreamSampler.for_lgcn(g), g.sample, 30, seed=n_items)
    g.batch_size = 8                                                     # (12 test users: sample needs B <= n_pop)
    check_equal(ReferenceStreamSampler.for_lgcn(g, test=True, batch_size=8), g.sample_test, 30, seed=n_items)


@pytest.mark.parametrize("B,n_pop", [(5, 21), (5, 22), (6, 85), (6, 86), (1024, 4117), (1024, 4118)])
def test_both_sides_of_random_sample_setsize(B, n_pop):
    """n_pop <= setsize: the pool form of random.sample; one more: the set form.  The LightGCN population has gaps and is
    shuffled, so a drawn index is not a user id."""
    rs = np.random.RandomState(B + n_pop)
    n_items, n = 50, 6 if B > 100 else 40
    lists = {u: rs.randint(0, n_items - 1, size=1 + u % 4).tolist() for u in range(n_pop)}
    d = synth_mf(lists, n_pop, n_items, B)
    check_equal(ReferenceStreamSampler.for_mf(d), d.sample, n, seed=n_pop)
    ids = rs.permutation(2 * n_pop + 3)[:n_pop].tolist()                  # gaps, shuffled
    assert ids != sorted(ids) and max(ids) >= n_pop
    glists = {u: rs.randint(0, n_items - 1, size=1 + u % 4).tolist() for u in ids}
    g = synth_lgcn(glists, ids, max(ids) + 1, n_items, B)
    check_equal(ReferenceStreamSampler.for_lgcn(g), g.sample, n, seed=n_pop)


def test_choice_path_when_the_batch_exceeds_n_users():
    rs = np.random.RandomState(3)
    n_users, n_items, B = 10, 40, 16
    lists = {u: rs.randint(0, n_items - 1, size=2 + u).tolist() for u in range(n_users)}
    d = synth_mf(lists, n_users, n_items, B)
    want = check_equal(ReferenceStreamSampler.for_mf(d), d.sample, 25)
    assert any(len(set(b[0])) < B for b in want)                          # drawn with replacement
    ids = [9, 2, 7, 0, 4]
    g = synth_lgcn({u: lists[u] for u in ids}, ids, n_users, n_items, B, {u: [u, u + 1] for u in ids[:3]})
    check_equal(ReferenceStreamSampler.for_lgcn(g), g.sample, 25)
    check_equal(ReferenceStreamSampler.for_lgcn(g, test=True), g.sample_test, 25)


def test_lgcn_empty_positive_list_is_an_error_where_the_reference_raises():
    n_users, n_items, B = 6, 20, 4
    lists = {u: [1, 2, 3] for u in range(n_users) if u != 2}
    g = synth_lgcn(lists, range(n_users), n_users, n_items, B)
    seed_all(1, mid_block=True)
    with pytest.raises(KeyError):
        for _ in range(50):
            g.sample()
    seed_all(1, mid_block=True)
    before = states()
    with pytest.raises(_lib.MacrError) as e:
        ReferenceStreamSampler.for_lgcn(g).generate(50)
    assert e.value.code == _lib.E_INVALID and "user 2" in str(e.value) and "empty" in str(e.value)
    assert states() == before                                             # all or nothing


# ---- refusals: no hang, no draw ------------------------------------------------------------------------------------------
def raw_call(s, n, B=None, n_users=None, py_pos=624, np_pos=624, null=()):
    """macr_ref_sample_batches on sampler s's tables with chosen arguments -> (status, message, states untouched?)"""
    B = s.batch_size if B is None else B
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    py_key = np.arange(624, dtype=np.uint32) * 2654435761 % (2 ** 32 - 5)
    py_key = py_key.astype(np.uint32)
    np_key = py_key[::-1].copy()
    keys0 = (py_key.copy(), np_key.copy())
    pp, npp = ctypes.c_int(py_pos), ctypes.c_int(np_pos)
    out = np.full((max(n, 0), 3, max(B, 1)), -7, dtype=np.int32)
    ptr = {"pop": p(s.pop), "pos_ptr": p(s.pos_ptr), "pos_idx": p(s.pos_idx), "excl_ptr": p(s.excl_ptr),
           "excl_idx": p(s.excl_idx), "py_key": p(py_key), "np_key": p(np_key), "out": p(out), "ws": p(s._ws),
           "py_pos": ctypes.byref(pp), "np_pos": ctypes.byref(npp)}
    for k in null:
        ptr[k] = None
    L = _lib.lib()
    rc = L.macr_ref_sample_batches(s.kind, n, B, s.n_users if n_users is None else n_users, ptr["pop"], len(s.pop),
                                   ptr["pos_ptr"], ptr["pos_idx"], ptr["excl_ptr"], ptr["excl_idx"], s.n_items, ptr["py_key"],
                                   ptr["py_pos"], ptr["np_key"], ptr["np_pos"], ptr["out"], ptr["ws"], s._ws.nbytes)
    untouched = (np.array_equal(py_key, keys0[0]) and np.array_equal(np_key, keys0[1]) and pp.value == py_pos
                 and npp.value == np_pos and (out == -7).all())
    return rc, L.macr_last_error().decode(), untouched


def test_refusals_leave_states_and_output_untouched():
    n_users, n_items = 12, 9
    lists = {u: [u % 8, 8] for u in range(n_users)}
    mf = ReferenceStreamSampler.for_mf(synth_mf(lists, n_users, n_items, 4))
    lg = ReferenceStreamSampler.for_lgcn(synth_lgcn(lists, range(n_users), n_users, n_items, 4))
    for s in (mf, lg):
        assert raw_call(s, 3)[::2] == (_lib.OK, False)                    # the same call with nothing wrong draws
        for name in ("pop", "pos_ptr", "pos_idx", "excl_ptr", "excl_idx", "py_key", "py_pos", "np_key", "np_pos", "out"):
            rc, msg, untouched = raw_call(s, 3, null=(name,))
            assert rc == _lib.E_INVALID and "null pointer" in msg and name in msg and untouched, (name, msg)
        rc, msg, untouched = raw_call(s, 3, null=("ws",))
        assert rc == _lib.E_WORKSPACE and "workspace" in msg and untouched
        for B in (0, -3):
            rc, msg, untouched = raw_call(s, 3, B=B)
            assert rc == _lib.E_INVALID and "B=%d" % B in msg and untouched
        for which, pos in (("py_pos", -1), ("py_pos", 625), ("np_pos", -1), ("np_pos", 625)):
            rc, msg, untouched = raw_call(s, 3, **{which: pos})
            assert rc == _lib.E_INVALID and "%s=%d" % (which, pos) in msg and untouched, msg
        # B <= n_users with B > n_pop: random.sample raises "Sample larger than population" (sample_test with few keys)
        rc, msg, untouched = raw_call(s, 3, B=13, n_users=13)
        assert rc == _lib.E_INVALID and "n_pop=12" in msg and "B=13" in msg and untouched
    # an exclusion list that covers the catalogue: the reference's rejection loop never ends; here refused, at once
    full = dict(lists)
    full[5] = list(range(n_items))[::-1]
    for s in (ReferenceStreamSampler.for_mf(synth_mf(full, n_users, n_items, 4)),
              ReferenceStreamSampler.for_lgcn(synth_lgcn(full, range(n_users), n_users, n_items, 4))):
        rc, msg, untouched = raw_call(s, 3)
        assert rc == _lib.E_INVALID and "user 5" in msg and "n_items=9" in msg and untouched, msg
        seed_all(9, mid_block=True)
        before = states()
        with pytest.raises(_lib.MacrError):
            s.generate(3)
        assert states() == before
    with pytest.raises(ValueError):                                       # the reference, for the record
        random.sample(range(12), 13)


# ---- the CLIs' train_epoch, without a GPU ---------------------------------------------------------------------------------
_CLI_CODE = r'''
import random, sys
import numpy as np
sys.argv = [%(script)r, "--data_path", %(data)r, "--dataset", "addressa", "--batch_size", "1024"]
sys.path.insert(0, %(cli_dir)r)
import %(module)s as cli
from macr_amd.host_sampler import ReferenceStreamSampler
class FakeLog(list):
    def __getitem__(self, k):
        return self if isinstance(k, slice) else None
    def cpu(self): return self
    def numpy(self): return np.zeros((3, 3))
class FakeModel(object):
    def __init__(self): self.batches = []
    def to_device_batch(self, u, i, j): return np.asarray([u, i, j], dtype=np.int32)
    def train_step(self, kind, batch, out, **kw): self.batches.append(np.array(batch, dtype=np.int32))
    def sync(self): pass
def states():
    a, b = random.getstate(), np.random.get_state()
    return a, (b[0], b[1].tobytes(), int(b[2]), int(b[3]), float(b[4]))
def seed():
    random.seed(11); np.random.seed(11); random.gauss(0, 1); np.random.standard_normal(1)
ok = []
for kw, sampler in %(cases)s:
    seed(); plain = FakeModel(); cli.train_epoch(plain, 0, 3, FakeLog(), **kw); want = states()
    seed(); fast = FakeModel(); cli.train_epoch(fast, 0, 3, FakeLog(), sampler(), **kw)
    ok.append(states() == want and len(fast.batches) == 3 and all(np.array_equal(a, b) for a, b in zip(plain.batches, fast.batches)))
print("RESULT", ok)
'''


@pytest.mark.parametrize("cli", ["mf", "lgcn"])
def test_train_epoch_with_the_native_sampler_leaves_the_states_of_the_sampler_less_call(cli):
    """train_epoch(FakeModel, ..., sampler) with a host-tensor ReferenceStreamSampler: the same three batches reach the
    model and the live states end where the sampler-less call leaves them -- for LightGCN that includes the discarded
    look-ahead batch (a pass is n_batch + 1), for the training pass and for the test-loss pass.  In a subprocess: the CLI
    modules parse sys.argv and load the dataset at import."""
    if cli == "mf":
        sub = dict(script="train.py", cli_dir=os.path.join(REPO, "macr_mf"), module="train",
                   cases="[({}, lambda: ReferenceStreamSampler.for_mf(cli.data))]")
    else:
        sub = dict(script="LightGCN.py", cli_dir=os.path.join(REPO, "macr_lightgcn"), module="LightGCN",
                   cases="[({}, lambda: ReferenceStreamSampler.for_lgcn(cli.data_generator)), "
                         "({'test_loss': True}, lambda: ReferenceStreamSampler.for_lgcn(cli.data_generator, test=True))]")
    sub["data"] = os.path.join(REPO, "data") + "/"
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", _CLI_CODE % sub], capture_output=True, text=True, timeout=300, env=env,
                         cwd=sub["cli_dir"])
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "RESULT " + str([True] * (1 if cli == "mf" else 2)), out.stdout[-2000:]


# ---- the core alone, under the host sanitizers --------------------------------------------------------------------------
def _case(s, n, fn, seed, chunk, expect_rc=0):
    """one case of tools/ref_sampler_check.cpp's file: sampler s's tables, the seeded states, and what the Python form
    `fn` makes of them"""
    seed_all(seed, mid_block=True)
    (_, internal, _), (_, np_keys, np_pos, _, _) = states()
    py_key = np.array(internal[:624], dtype=np.uint32)
    np_key = np.frombuffer(np_keys, dtype=np.uint32)
    head = [s.kind, n, s.batch_size, s.n_users, len(s.pop), s.n_items, len(s.pos_idx), len(s.excl_idx), internal[624], np_pos,
            expect_rc, chunk]
    parts = [np.asarray(head, dtype=np.int32), s.pop, s.pos_ptr, s.pos_idx, s.excl_ptr, s.excl_idx, py_key, np_key]
    if expect_rc == 0:
        parts.append(python_form(fn, n))
        (_, internal, _), (_, np_keys, np_pos, _, _) = states()
        parts += [np.array(internal, dtype=np.uint32), np.frombuffer(np_keys, dtype=np.uint32),
                  np.asarray([np_pos], dtype=np.uint32)]
    return b"".join(np.ascontiguousarray(p).astype("<u4" if p.dtype == np.uint32 else "<i4").tobytes() for p in parts)


def test_core_alone_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tools/ref_sampler_check.cpp: a plain C++ main around ref_sampler_core.hpp, built with g++ -fsanitize=address,undefined
    and run on cases written here -- the edge cases above folded in, every array in a heap block of exactly its size.
    (Both runtimes linked statically: the program then runs the same whatever else the environment loads into it.)"""
    cases = []
    rs = np.random.RandomState(42)
    for n_items in (2, 257, 744):
        lists = edge_lists(24, n_items, rs, with_empty=True)
        d = synth_mf(lists, 24, n_items, 16)
        cases.append(_case(ReferenceStreamSampler.for_mf(d), 12, d.sample, n_items, 5))
        lists = edge_lists(24, n_items, rs, with_empty=False)
        tests = {u: rs.randint(0, n_items - 1, size=1 + u % 3).tolist() for u in range(0, 24, 2) if u != 9}
        g = synth_lgcn(lists, rs.permutation(24).tolist(), 24, n_items, 8, tests)
        cases.append(_case(ReferenceStreamSampler.for_lgcn(g), 12, g.sample, n_items, 12))
        cases.append(_case(ReferenceStreamSampler.for_lgcn(g, test=True), 12, g.sample_test, n_items, 1))
    for B, n_pop in ((5, 21), (5, 22), (6, 85), (6, 86), (1024, 4117), (1024, 4118)):      # pool form | set form
        ids = rs.permutation(2 * n_pop)[:n_pop].tolist()
        g = synth_lgcn({u: rs.randint(0, 49, size=1 + u % 4).tolist() for u in ids}, ids, max(ids) + 1, 50, B)
        cases.append(_case(ReferenceStreamSampler.for_lgcn(g), 3, g.sample, n_pop, 2))
    lists = {u: rs.randint(0, 39, size=2 + u).tolist() for u in range(10)}
    d = synth_mf(lists, 10, 40, 16)                                         # B > n_users: the choice path
    cases.append(_case(ReferenceStreamSampler.for_mf(d), 9, d.sample, 1, 4))
    full = dict(lists)
    full[3] = list(range(40))                                               # refused: covers the catalogue
    cases.append(_case(ReferenceStreamSampler.for_mf(synth_mf(full, 10, 40, 4)), 3, None, 1, 3, expect_rc=_lib.E_INVALID))
    g = synth_lgcn({u: [1, 2] for u in range(10) if u != 4}, range(10), 10, 40, 4)   # refused at the draw: empty list
    cases.append(_case(ReferenceStreamSampler.for_lgcn(g), 40, None, 1, 40, expect_rc=_lib.E_INVALID))
    # and the real thing, over several twists
    cases.append(_case(ReferenceStreamSampler.for_mf(mf_data("addressa")), 4, mf_data("addressa").sample, 7, 3))
    path = tmp_path / "cases.bin"
    path.write_bytes(b"RSC1" + np.asarray([len(cases)], dtype="<i4").tobytes() + b"".join(cases))

    exe = str(tmp_path / "ref_sampler_check")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(REPO, "tools", "ref_sampler_check.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "%d cases ok" % len(cases) in run.stdout
    bad = bytearray(path.read_bytes())                                     # the checker does notice a difference
    bad[-8] ^= 1
    path.write_bytes(bytes(bad))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and "state differs" in run.stderr, run.stderr[-2000:]
