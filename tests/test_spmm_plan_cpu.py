"""The SpMM plan (macr_spmm_plan_build, macr_amd/csrc/spmm_kernels.hip) decoded on the host: both schedules -- the row items
with their pieces, groups and records, and the entry stream -- must describe the matrix completely and consistently under
every plan-time knob, the knobs are read per plan (not latched by the first plan of the process), and the graphs of
tests/test_gpu_spmm_hubs.py keep the group-count edges its cases are built for.  No GPU."""
import numpy as np
import pytest

import spmm_cases as sc

SETTINGS = {
    "defaults": {},
    "octants0": {"MACR_SPMM_OCTANTS": "0"},
    "chunk64": {"MACR_SPMM_CHUNK": "64"},
    "chunk64_octants0": {"MACR_SPMM_CHUNK": "64", "MACR_SPMM_OCTANTS": "0"},
    "stream": {"MACR_SPMM_STREAM": "1"},
    "stream_hub32_t32": {"MACR_SPMM_STREAM": "1", "MACR_SPMM_HUB": "32", "MACR_SPMM_T": "32"},
    "stream_octants0": {"MACR_SPMM_STREAM": "1", "MACR_SPMM_OCTANTS": "0"},
}
GRAPHS = {"small": sc.small, "deep": sc.deep, "sparse": sc.sparse_graph, "isolated": sc.isolated, "star": sc.star}


@pytest.fixture(scope="module")
def lib():
    from macr_amd import _lib
    return _lib.lib()


def set_knobs(monkeypatch, env):
    for name in sc.PLAN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def source_ranges(A, hub):
    """eight ranges of source rows of equal entry mass over the rows longer than `hub`: bound[x] is one past the first
    column at which the running mass reaches x eighths"""
    deg = np.diff(A.indptr)
    N = A.shape[0]
    mass = np.bincount(A.indices[np.repeat(deg > hub, deg)], minlength=N).astype(np.int64)
    cum, total = np.cumsum(mass), int(mass.sum())
    bound = [0]
    for x in range(1, 8):
        c = int(np.searchsorted(cum * 8, total * x, side="left"))
        bound.append(c + 1 if c < N else N)
    return np.asarray(bound + [N])


def check_groups(t, hub_rows):
    """the group tables of either schedule: groups are at most kGroup consecutive slots of one hub row, and the five
    arrays say the same thing"""
    n_slots, n_groups, n_split = t["n_slots"], t["n_groups"], t["n_split"]
    assert len(t["slot_group"]) == n_slots and len(t["group_slot0"]) == n_groups + 1
    assert len(t["group_split"]) == n_groups and len(t["split_group0"]) == n_split + 1 and len(t["split_row"]) == n_split
    assert np.array_equal(t["split_row"], hub_rows)
    gs0, sg0 = t["group_slot0"].astype(np.int64), t["split_group0"].astype(np.int64)
    assert gs0[0] == 0 and gs0[-1] == n_slots and sg0[0] == 0 and sg0[-1] == n_groups
    sizes = np.diff(gs0)
    if n_groups:
        assert sizes.min() >= 1 and sizes.max() <= sc.K_GROUP
    assert np.all(np.diff(sg0) >= 1)
    assert np.array_equal(t["slot_group"], np.repeat(np.arange(n_groups), sizes))
    assert np.array_equal(t["group_split"], np.repeat(np.arange(n_split), np.diff(sg0)))
    last_of_row = np.zeros(n_groups, bool)
    last_of_row[sg0[1:] - 1] = True
    assert np.all(sizes[~last_of_row] == sc.K_GROUP)             # only a row's last group may be short


def check_row_plan(P, A, env):
    rowptr, col = A.indptr.astype(np.int64), A.indices
    N = A.shape[0]
    deg = np.diff(rowptr)
    chunk = int(env.get("MACR_SPMM_CHUNK", 512))
    octants = env.get("MACR_SPMM_OCTANTS", "1") != "0"
    assert P["N"] == N and P["chunk"] == chunk
    hub_rows = np.flatnonzero(deg > chunk)
    items = P["items"].astype(np.int64)
    n_slots = P["n_slots"]
    assert len(items) == P["n_items"] == n_slots + N - len(hub_rows)
    check_groups(P, hub_rows)
    # pieces: the first n_slots items; every slot once; in slot order they tile their rows
    pieces = items[:n_slots]
    assert np.array_equal(np.sort(pieces[:, 3]), np.arange(n_slots))
    pieces = pieces[np.argsort(pieces[:, 3])]
    if not octants:
        assert np.array_equal(P["items"][:n_slots, 3], np.arange(n_slots))   # launched in slot order
    owner = P["split_row"][P["group_split"][P["slot_group"]]] if n_slots else np.zeros(0, np.int64)
    assert np.array_equal(pieces[:, 0], owner)
    length = pieces[:, 2] - pieces[:, 1]
    if n_slots:
        assert length.min() >= 1 and length.max() <= chunk
    first = np.r_[True, owner[1:] != owner[:-1]] if n_slots else np.zeros(0, bool)
    last = np.r_[owner[1:] != owner[:-1], True] if n_slots else np.zeros(0, bool)
    assert np.array_equal(pieces[first, 1], rowptr[hub_rows]) and np.array_equal(pieces[last, 2], rowptr[hub_rows + 1])
    assert np.array_equal(pieces[1:, 1][~first[1:]], pieces[:-1, 2][~last[:-1]])
    if octants and n_slots:
        bound = source_ranges(A, chunk)
        lo = np.searchsorted(bound, col[pieces[:, 1]], side="right")
        hi = np.searchsorted(bound, col[pieces[:, 2] - 1], side="right")
        assert np.array_equal(lo, hi)                           # (columns ascend inside a row)
        # a piece ends at the chunk size, at the row's end or at a range boundary -- nowhere else
        full = (length == chunk) | last
        nxt = np.searchsorted(bound, col[np.minimum(pieces[:, 2], len(col) - 1)], side="right")
        assert np.all(full | (nxt > hi))
    elif n_slots:
        assert np.all((length == chunk) | last)
    # the other rows: once each, slot -1, longest first
    rest = items[n_slots:]
    assert np.all(rest[:, 3] == -1)
    assert np.array_equal(np.sort(rest[:, 0]), np.flatnonzero(deg <= chunk))
    assert np.array_equal(rest[:, 1], rowptr[rest[:, 0]]) and np.array_equal(rest[:, 2], rowptr[rest[:, 0] + 1])
    rl = rest[:, 2] - rest[:, 1]
    assert np.all(np.diff(rl) <= 0)
    assert P["n_single"] == n_slots + int((rl > sc.REC_ENTRIES).sum())
    return hub_rows


def check_records(P, A):
    rowptr, col, val = A.indptr.astype(np.int64), A.indices, A.data.view(np.uint32)
    short = P["items"][P["n_single"]:, 0]
    seen = []
    for c, (rows, cols, w) in enumerate(P["records"]):
        R, E = 8 >> c, sc.REC_ENTRIES // (8 >> c)
        assert len(rows) == P["n_rec"][c]
        assert np.all(rows[:, R:] == -1)
        r = rows[:, :R].astype(np.int64)
        ok = r >= 0
        beg = rowptr[np.maximum(r, 0)]
        n = np.where(ok, rowptr[np.maximum(r, 0) + 1] - beg, 0)
        assert np.all(n <= E)
        if c:
            assert np.all(n[ok] > E // 2)                       # (a shorter row belongs to the class before)
        e = np.arange(E)
        live = e[None, None, :] < n[:, :, None]
        src = np.minimum(beg[:, :, None] + e, len(col) - 1)
        assert np.array_equal(cols[live], col[src][live]) and np.array_equal(w.view(np.uint32)[live], val[src][live])
        assert np.all(cols[~live] == 0) and np.all(w.view(np.uint32)[~live] == 0)      # padding weighs 0
        seen.append(r[ok])
    seen = np.concatenate(seen) if seen else np.zeros(0, np.int64)
    assert np.array_equal(np.sort(seen), np.sort(short))         # every short row in exactly one record
    assert np.all(np.diff(rowptr)[short] <= sc.REC_ENTRIES)


def check_stream(S, A, env):
    rowptr, col, val = A.indptr.astype(np.int64), A.indices, A.data.view(np.uint32)
    deg = np.diff(rowptr)
    hub = int(env.get("MACR_SPMM_HUB", 512))
    octants = env.get("MACR_SPMM_OCTANTS", "1") != "0"
    hub_rows = np.flatnonzero(deg > hub)
    check_groups(S, hub_rows)
    pc, pw = S["pc"], S["pw"].view(np.uint32)
    E = S["n_entries"]
    assert E == 32 * S["n_sb"] and np.all(S["tail"] == 0) and len(S["tail"]) == 128
    # chunk descriptors: every sub-batch once
    ch = S["chunks"].astype(np.int64)
    # (behind the chunks: descriptors without entries, which only carry a share of the empties -- present exactly when the
    # chunks are too few to name all of them, 255 to a descriptor)
    bare = ch[:, 0] == ch[:, 1]
    n_real = int((~bare).sum())
    assert not bare[:n_real].any() and np.all(ch[bare, 3] == -1) and np.all(ch[bare, 0] == S["n_sb"])
    assert len(ch) == max(n_real, (S["n_empty"] + 254) // 255)
    # the empties: exactly the rows without neighbours, shared out without overlap (in descriptor order)
    assert np.array_equal(S["empties"], np.flatnonzero(deg == 0)) and S["n_empty"] < 1 << 24
    e_first, e_cnt = ch[:, 2] & 0xffffff, (ch[:, 2] >> 24) & 0xff
    assert np.array_equal(e_first, np.r_[0, np.cumsum(e_cnt)[:-1]]) and e_cnt.sum() == S["n_empty"]
    ch = ch[:n_real]
    order = np.argsort(ch[:, 0], kind="stable")
    sb0, sb1, slot = ch[order, 0], ch[order, 1], ch[order, 3]
    assert np.all(sb1 > sb0) and sb0[0] == 0 and sb1[-1] == S["n_sb"] and np.array_equal(sb0[1:], sb1[:-1])
    # entries: markers close a row (weight word 0) or a piece (1), only as the last entry of a group of 8
    marker = pc < 0
    at = np.flatnonzero(marker)
    assert np.all(at % 8 == 7) and np.all(pw[at] <= 1)
    mrow = (pc[at] & 0x7fffffff).astype(np.int64)
    real = ~marker & (pw != 0)
    pad = ~marker & (pw == 0)
    # walking the stream reproduces the matrix entry by entry, in row order
    assert np.array_equal(pc[real], col) and np.array_equal(pw[real], val)
    before = np.r_[0, np.cumsum(real)]                          # real entries in front of position e
    seg_beg, seg_end = before[np.r_[0, at[:-1] + 1]], before[at]
    is_row = pw[at] == 0
    assert np.array_equal(seg_beg[is_row], rowptr[mrow[is_row]]) and np.array_equal(seg_end[is_row], rowptr[mrow[is_row] + 1])
    assert np.all(deg[mrow[is_row]] <= hub) and np.all(deg[mrow[is_row]] > 0)
    assert np.array_equal(mrow[is_row], np.flatnonzero((deg > 0) & (deg <= hub)))      # each once, in row order
    pl = (seg_end - seg_beg)[~is_row]
    prow = mrow[~is_row]
    assert len(pl) == S["n_slots"]
    if len(pl):
        assert pl.min() >= 1 and pl.max() <= sc.STREAM_PIECE - 1
    assert np.array_equal(prow, S["split_row"][S["group_split"][S["slot_group"]]])       # pieces in slot order, row by row
    assert np.all(seg_beg[~is_row] >= rowptr[prow]) and np.all(seg_end[~is_row] <= rowptr[prow + 1])
    # (with the entry-by-entry equality above: the pieces of a row tile it)
    # chunks: a piece is a chunk of its own that ends with the piece marker; the others hold whole rows
    chunk_of = np.searchsorted(sb0 * 32, np.arange(E), side="right") - 1
    m_chunk = chunk_of[at]
    assert np.array_equal(slot[m_chunk[~is_row]], np.arange(S["n_slots"]))
    assert np.all(slot[m_chunk[is_row]] == -1)
    assert np.array_equal(np.sort(slot[slot >= 0]), np.arange(S["n_slots"]))
    assert np.all(np.bincount(m_chunk[~is_row], minlength=len(sb0))[slot >= 0] == 1)
    assert np.all((sb1 - sb0)[slot >= 0] * 32 <= sc.STREAM_PIECE)
    # padding: in front of a marker in the marker's group of 8 (gathers the marker's row), or behind the chunk's last marker
    nxt = np.searchsorted(at, np.arange(E), side="left")        # index into `at` of the next marker at or behind e
    nxt_pos = np.where(nxt < len(at), at[np.minimum(nxt, len(at) - 1)], E)
    chunk_end = sb1[chunk_of] * 32
    assert np.all(nxt_pos[real] < chunk_end[real])               # every entry is followed by a marker of its own chunk
    p = np.flatnonzero(pad)
    same_group = nxt_pos[p] // 8 == p // 8
    assert np.array_equal(pc[p[same_group]], mrow[nxt[p[same_group]]])
    trailing = p[~same_group]
    assert np.all(nxt_pos[trailing] >= chunk_end[trailing]) and np.all(pc[trailing] == 0)
    if octants and len(pl):
        bound = source_ranges(A, hub)
        b, e = seg_beg[~is_row], seg_end[~is_row]
        assert np.array_equal(np.searchsorted(bound, col[b], side="right"), np.searchsorted(bound, col[e - 1], side="right"))
    elif len(pl):
        last = np.r_[prow[1:] != prow[:-1], True]
        assert np.all((pl == sc.STREAM_PIECE - 1) | last)


_plans = {}


def plan_of(lib, monkeypatch, graph, setting):
    set_knobs(monkeypatch, SETTINGS[setting])
    if (graph, setting) not in _plans:
        _plans[graph, setting] = sc.build_plan_host(GRAPHS[graph](), lib)
    return _plans[graph, setting]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_plan_describes_the_matrix(lib, monkeypatch, graph, setting):
    env = SETTINGS[setting]
    A = GRAPHS[graph]()
    host = plan_of(lib, monkeypatch, graph, setting)
    P = sc.decode_plan(host)
    check_row_plan(P, A, env)
    check_records(P, A)
    assert sum(P["n_rec"]) * sc.REC_INTS == P["end_of_records"] - P["rec_off"]
    want_stream = env.get("MACR_SPMM_STREAM") == "1"
    assert (P["stream"] is not None) == want_stream
    if want_stream:
        assert P["reserved"] == (P["end_of_records"] + 15) // 16 * 16
        check_stream(P["stream"], A, env)
    else:
        assert P["end_of_records"] == len(host)
    if graph == "sparse":
        assert int((np.diff(A.indptr) == 0).sum()) == 10 and P["n_split"] >= 5
    if graph == "isolated" and setting == "stream":             # more rows without neighbours than the chunks can name
        S = P["stream"]
        assert S["n_empty"] >= 20000 > 255 * int((S["chunks"][:, 0] != S["chunks"][:, 1]).sum())


def test_plan_knobs_are_read_per_plan(lib, monkeypatch):
    """Each of the four plan-time knobs, flipped IN THIS PROCESS after a plan has been built, changes the next plan, and
    flipping it back reproduces the first plan byte for byte; plan_bytes and plan_build agree throughout (build_plan_host
    asserts it).  Before the knobs were read per plan build the first plan of the process fixed all four."""
    A = sc.small()
    base_env = {"MACR_SPMM_STREAM": "1"}
    set_knobs(monkeypatch, base_env)
    base = sc.build_plan_host(A, lib)
    for knob, value in (("MACR_SPMM_CHUNK", "64"), ("MACR_SPMM_OCTANTS", "0"), ("MACR_SPMM_HUB", "32"), ("MACR_SPMM_T", "32")):
        monkeypatch.setenv(knob, value)
        flipped = sc.build_plan_host(A, lib)
        assert len(flipped) != len(base) or not np.array_equal(flipped, base), knob
        monkeypatch.delenv(knob)
        again = sc.build_plan_host(A, lib)
        assert np.array_equal(again, base), knob
    # out-of-range values keep the defaults, as before
    for knob, value in (("MACR_SPMM_CHUNK", "63"), ("MACR_SPMM_HUB", "31"), ("MACR_SPMM_T", "31")):
        monkeypatch.setenv(knob, value)
        assert np.array_equal(sc.build_plan_host(A, lib), base), knob
        monkeypatch.delenv(knob)
    monkeypatch.setenv("MACR_SPMM_STREAM", "0")
    assert sc.decode_plan(sc.build_plan_host(A, lib))["stream"] is None


def test_graphs_keep_their_group_count_edges(lib, monkeypatch):
    """The cases of tests/test_gpu_spmm_hubs.py rest on these counts: a default that moves must not silently take a
    reduction branch out of the GPU tests."""
    deg = lambda A: np.diff(A.indptr)
    n_u = sc.SMALL_SHAPE[0]
    assert sc.small().shape[0] == 9064 and [int(deg(sc.small())[n_u + h]) for h, _ in sc.SMALL_HUBS] == [n for _, n in sc.SMALL_HUBS]
    assert sc.deep().shape[0] == 140064 and int(deg(sc.deep())[sc.DEEP_SHAPE[0]:].min()) > 512      # all 64 items are hubs
    P = sc.decode_plan(plan_of(lib, monkeypatch, "small", "octants0"))
    # exactly one full group (8 192) -- full group + a group of ONE piece (8 193; 8 704) -- two pieces (513) -- 16 + 2 (9 000)
    assert sc.group_sizes(P) == [16, 16, 1, 16, 1, 2, 16, 2]
    P = sc.decode_plan(plan_of(lib, monkeypatch, "small", "defaults"))
    assert sc.group_sizes(P) == sc.SMALL_GROUPS_OCTANTS
    assert int((P["items"][:P["n_slots"], 2] - P["items"][:P["n_slots"], 1]).min()) == 1     # the smallest piece: one entry
    S = sc.decode_plan(plan_of(lib, monkeypatch, "small", "stream"))["stream"]
    assert (S["n_slots"], S["n_groups"]) == (164, 13)
    assert 1 in sc.group_sizes(S) or min(sc.group_sizes(S)) < sc.K_GROUP
    P = sc.decode_plan(plan_of(lib, monkeypatch, "small", "chunk64"))
    assert max(sc.groups_per_row(P).values()) >= 9 and P["n_split"] > 5       # many groups per row, the 150-neighbour items are hubs too
    P = sc.decode_plan(plan_of(lib, monkeypatch, "deep", "defaults"))
    n_u = sc.DEEP_SHAPE[0]
    per_row = sc.groups_per_row(P)
    assert per_row[n_u + 0] == 17 and per_row[n_u + 1] == 9     # more than kGroup groups: the second level takes two rounds
    S = sc.decode_plan(plan_of(lib, monkeypatch, "deep", "stream"))["stream"]
    assert sc.groups_per_row(S)[n_u + 0] > 2 * sc.K_GROUP and sc.groups_per_row(S)[n_u + 1] > sc.K_GROUP
    assert S["n_groups"] == 113
    # STAR (exact at four layers): ONE hub row of 520 entries, just past the split threshold -- two pieces in slot order, eight
    # short ones cut at the source ranges (the default), nine / sixteen of at most 64 entries; always a single group
    n_u = sc.STAR_SHAPE[0]
    assert sc.star().shape[0] == 680 and int(deg(sc.star())[n_u]) == sc.STAR_HUB > 512 > int(deg(sc.star())[n_u + 1:].max())
    for setting, pieces in (("octants0", 2), ("defaults", 8), ("chunk64_octants0", 9), ("chunk64", 16)):
        P = sc.decode_plan(plan_of(lib, monkeypatch, "star", setting))
        assert sc.group_sizes(P) == [pieces] and sc.groups_per_row(P) == {n_u: 1}, setting
    S = sc.decode_plan(plan_of(lib, monkeypatch, "star", "stream"))["stream"]
    assert sc.group_sizes(S) == [8] and sc.groups_per_row(S) == {n_u: 1}
