"""Prescribed layouts of the sorted reference list for the staged gradient path, with an exact integer reference.

Above 8192 triples, and in every deterministic and row-sharded step, a gradient row is the sum of its staged rows: the 3B
references of a batch are keyed by row (k_refs_init / k_shard_keys, macr_amd/csrc/train_kernels.hip), radix-sorted
(refsort.hpp) and summed per row by one of four reductions -- k_seg_reduce (atomics for runs cut into chunks), k_seg_scan +
k_seg_sum (INDEX mode: flags that name short runs, work items for long ones), k_seg_reduce<., true> + k_seg_fold (ordered slots)
and k_seg_reduce_inv + k_seg_fold_inv (slots cut at the run's start).  All of it is index arithmetic, and a mistake is one lost,
doubled or mis-owned reference -- which whole training steps compared with a tolerance do not see.

A case here is a list of (row, run length) pairs per table in ascending key order, so where every run lies in the SORTED list is
known before anything runs: its offset in the window of CH positions, its place against the 256 / LPR positions of a block,
whether it ends the list.  The batch is a fixed shuffle of those references.  The staging rows hold integers in [-7, 7]: as long
as max over rows of sum |terms| < 2^24, every partial sum of every order and shape is an integer below 2^24 and fp32 addition is
exact -- atomics included -- so the GPU result must equal the int64 sum BIT FOR BIT (tests/test_gpu_seg_exact.py).  layout()
restates in numpy what the kernels decide for each run (heads, slots, chunk counts, flags, work items), read off their code;
tests/test_seg_cases_cpu.py shows without a GPU that every case contains the feature it exists for.
"""
import numpy as np

DIMS = (32, 64, 128, 256)
MODES = ("reduce", "index", "det", "inv")
K_REF_SHIFT, K_REF_RUN, K_LONG_SPAN = 26, 16, 64         # kRefShift, kRefRun, kLongSpan of train_kernels.hip
STAGE_MAX = 7                                            # |entries| of the staging rows
NAN_BITS = np.uint32(0x7FC00000)                         # rows the kernels STORE start as this NaN
FLAG_INIT = np.int32(0x5A5A5A5A)                         # row flags start as this; no kernel writes it
GUARD_ROWS = 2                                           # rows behind each table: where a key >= key_end taken for a row would land


def ch_of(d):
    """CH of k_seg_reduce: positions per window"""
    return min(d // 4, 16)


def rpb_of(d):
    """positions per block of k_seg_reduce / k_seg_fold: 256 / LPR"""
    return 256 // (d // 4)


def lens_of(d):
    CH = ch_of(d)
    out = []
    for L in (1, CH - 1, CH, CH + 1, 16, 17, 2 * CH, 2 * CH + 1, 63, 64, 65, 128, 129):
        if L not in out:
            out.append(L)
    return out


# ---- case descriptions -----------------------------------------------------------------------------------------------------
# A table's part of the sorted list is written as directives, laid out from the position the part begins at:
#   ("run", L, tag)     a row with L references (tag: what the CPU test must find there)
#   ("at", m, r)        single-reference rows until position % m == r
#   ("singles", k)      k single-reference rows
# and a `*_tail`: runs that END the part (single-reference rows are put in front of them until the part has its size).
def _lay(directives, pos):
    runs = []
    for dv in directives:
        if dv[0] == "run":
            runs.append((dv[1], dv[2], pos))
            pos += dv[1]
        elif dv[0] == "at":
            while pos % dv[1] != dv[2] % dv[1]:
                runs.append((1, None, pos))
                pos += 1
        else:
            for _ in range(dv[1]):
                runs.append((1, None, pos))
                pos += 1
    return runs, pos


def _pad_and_tail(runs, pos, end, tail):
    need = sum(L for L, _ in tail)
    assert pos + need <= end, (pos, need, end)
    while pos + need < end:
        runs.append((1, None, pos))
        pos += 1
    for L, tag in tail:
        runs.append((L, tag, pos))
        pos += L
    return runs


def _spec(users=(), items=(), users_tail=(), items_tail=(), B_min=1, B_mod=None, own=None, foreign_min=0, n_loc_min=(1, 1)):
    return dict(users=list(users), items=list(items), users_tail=list(users_tail), items_tail=list(items_tail), B_min=B_min,
                B_mod=B_mod, own=own, foreign_min=foreign_min, n_loc_min=n_loc_min)


def _placed(d, offset):
    """every run length at window offset `offset`"""
    CH = ch_of(d)
    out = []
    for L in lens_of(d):
        out += [("at", CH, offset), ("run", L, dict(len=L, off=offset % CH))]
    return out


def _straddling(d):
    """every run length >= 2 across an edge of k_seg_reduce's block: once with only its first reference before the edge, once
    with only its last behind it"""
    R = rpb_of(d)
    out = []
    for L in lens_of(d):
        if L < 2:
            continue
        out += [("at", R, R - 1), ("run", L, dict(len=L, straddle=True))]
        out += [("at", R, (R - (L - 1)) % R), ("run", L, dict(len=L, straddle=True))]
    return out


def _nc_len(d, k, on_edge, off=3):
    """length of a run that begins at window offset `off` and has k following windows; on_edge: its end is a window's end"""
    CH = ch_of(d)
    return (CH - off) + (k * CH if on_edge else (k - 1) * CH + 2)


def _nc_runs(d, on_edge):
    CH = ch_of(d)
    out = []
    for k in range(1, 10):
        L = _nc_len(d, k, on_edge)
        out += [("at", CH, 3), ("run", L, dict(len=L, off=3, nc=k, ends_on_window=on_edge))]
    return out


_MIX = (1, 3, 17, 65, 2, 16, 33)


def _mix(d, last):
    CH = ch_of(d)
    out = []
    for k, L in enumerate(_MIX + (CH + 1, 2 * CH)):
        out += [("singles", k % 3), ("run", L, dict(len=L))]
    out += [("run", last, dict(len=last, last_owned=True))]
    return out


def _specs(d):
    CH = ch_of(d)
    big = 1000 * CH + 40                      # nc >= 1000 from any offset
    S = {}
    for name, off in (("lengths_off0", 0), ("lengths_off1", 1), ("lengths_offlast", CH - 1)):
        S[name] = _spec(users=_placed(d, off), items=_placed(d, off), B_mod=(32, 5))
    S["lengths_straddle"] = _spec(users=_straddling(d), items=_straddling(d), B_mod=(32, 11))
    S["nc_inside"] = _spec(users=_nc_runs(d, False), items=_nc_runs(d, False), B_mod=(32, 7))
    S["nc_window_edge"] = _spec(users=_nc_runs(d, True), items=_nc_runs(d, True), B_mod=(32, 9))
    for k in range(1, 10):
        # the LAST run of the list has k following windows (B % 16 = k: the last window is partial; k = 9: B % 16 = 0, it is full)
        S["nc_last_%d" % k] = _spec(users=[("run", 2, dict(len=2))], B_mod=(16, k % 9), B_min=16 * 12,
                                    items_tail=[(None, dict(nc=k, last=True, fold_hits_nwin=True))])
    S["nc_big_inside"] = _spec(items=[("at", CH, 3), ("run", big, dict(len=big, off=3, min_nc=1000, ends_on_window=False))],
                               users=[("at", CH, 5), ("run", 5 * CH, dict(len=5 * CH))], B_mod=(32, 3))
    S["nc_big_window_edge"] = _spec(items=[("at", CH, 3), ("run", 1001 * CH - 3, dict(len=1001 * CH - 3, off=3, min_nc=1000, ends_on_window=True))],
                                    B_mod=(32, 13))
    S["nc_big_last"] = _spec(users=[("run", 3, dict(len=3))], items_tail=[(big, dict(len=big, min_nc=1000, last=True, fold_hits_nwin=True))],
                             B_mod=(32, 21))
    # list edges: a long run at position 0, n a multiple of neither CH nor the block, the last user key and the first item key
    # long and adjacent, the list ending in a single reference
    S["list_edges"] = _spec(users=[("run", 129, dict(len=129, start=0))], users_tail=[(65, dict(len=65, last_user=True))],
                            items=[("run", 65, dict(len=65, first_item=True))], items_tail=[(40, dict(len=40)), (1, dict(len=1, last=True))],
                            B_mod=(32, 5), B_min=229)
    # INDEX capacity: 17 references give the most work items per reference; and every reference of the batch in a long run
    S["index_all_17"] = _spec(users=[("run", 17, dict(len=17))] * 24, items=[("run", 17, dict(len=17))] * 48, B_min=17 * 24)
    S["index_one_row"] = _spec(users_tail=[(715, dict(len=715, start=0))], items_tail=[(1430, dict(len=1430, last=True))], B_min=715)
    # ownership: the row-sharded step's keys (k_shard_keys): foreign references sort behind key_end, directly after a long owned run
    S["own_interleaved"] = _spec(users=_mix(d, 5), items=_mix(d, 129), own=dict(u=(1, 3), i=(2, 3)), foreign_min=9, B_mod=(32, 5))
    S["own_range"] = _spec(users=_mix(d, 2 * CH + 1), items=_mix(d, 65), own=dict(u=(50, 1), i=(30, 1)), foreign_min=9, B_mod=(32, 27))
    S["own_range_first"] = _spec(users=_mix(d, 17), items=_mix(d, 64), own=dict(u=(0, 1), i=(5, 1)), foreign_min=5, B_mod=(16, 3))
    S["own_no_users"] = _spec(items=_mix(d, 129), own=dict(u=(4, 3), i=(0, 3)), foreign_min=3, n_loc_min=(0, 1), B_mod=(32, 19))
    S["own_nothing"] = _spec(own=dict(u=(2, 3), i=(7, 1)), foreign_min=40, n_loc_min=(5, 6), B_mod=(16, 7))
    return S


CASE_NAMES = tuple(_specs(64))
CASE_IDS = tuple((d, name) for d in DIMS for name in CASE_NAMES)


def _bump(B, mod):
    if mod:
        while B % mod[0] != mod[1]:
            B += 1
    return B


def _rows_for(runs, n_loc_min):
    """local rows of a table's runs, ascending: row 0 first, an unreferenced row now and then, the last run on the last row"""
    rows, r = [], 0
    for k in range(len(runs)):
        rows.append(r)
        r += 1 + (1 if k % 4 == 2 else 0)
    n_loc = rows[-1] + 1 if rows else 0
    return rows, max(n_loc, n_loc_min)


_cache = {}


def case(d, name):
    """-> dict: d, B, n = 3B, owned = (u_lo, u_stride, n_users_loc, i_lo, i_stride, n_items_loc), sharded, u / i / j (int32[B]),
    stage (fp32[3B][d], integers), runs (every owned run as laid out: (table, start, len)), want (the tagged ones: (table, start,
    len, tag)), n_users / n_items (global table rows)."""
    if (d, name) in _cache:
        return _cache[(d, name)]
    sp = _specs(d)[name]
    CH = ch_of(d)
    own = sp["own"]
    if own is None:
        ur, upos = _lay(sp["users"], 0)
        utail = sum(L for L, _ in sp["users_tail"])
        B = _bump(max(upos + utail, sp["B_min"]), sp["B_mod"])
        while True:
            ir, ipos = _lay(sp["items"], B)
            tail = list(sp["items_tail"])
            if tail and tail[0][0] is None:                        # the last run sized for its nc: it begins at offset 3 of a window
                k = tail[0][1]["nc"]
                L = 3 * B - (((3 * B + CH - 1) // CH - 1 - k) * CH + 3)
                tail[0] = (L, dict(tail[0][1], len=L, off=3))
            need = ipos - B + sum(L for L, _ in tail)
            if need <= 2 * B:
                break
            B = _bump(max(B + 1, (need + 1) // 2), sp["B_mod"])
        users = _pad_and_tail(ur, upos, B, sp["users_tail"])
        items = _pad_and_tail(ir, ipos, 3 * B, tail)
        n_foreign_u = n_foreign_i = 0
    else:
        users, upos = _lay(sp["users"], 0)
        items, ipos = _lay(sp["items"], upos)
        B = _bump(max(upos, (ipos - upos + 1) // 2, sp["B_min"]) + sp["foreign_min"], sp["B_mod"])
        n_foreign_u, n_foreign_i = B - upos, 2 * B - (ipos - upos)
    urow, n_ul = _rows_for(users, sp["n_loc_min"][0])
    irow, n_il = _rows_for(items, sp["n_loc_min"][1])
    (u_lo, u_st), (i_lo, i_st) = (own["u"], own["i"]) if own else ((0, 1), (0, 1))
    owned = (u_lo, u_st, n_ul, i_lo, i_st, n_il)

    def refs_of(runs, rows, lo, st, n_loc, n_foreign):
        out = []
        for (L, _, _), r in zip(runs, rows):
            out += [lo + r * st] * L
        # rows of other ranks: just before the range, just behind it (lo + n_loc * stride: the right residue, one row too far),
        # a neighbour's residue, and row 0
        foreign = [lo + n_loc * st, lo + n_loc * st + 1] + ([lo - 1, 0] if lo > 0 else []) + ([lo + 1, lo + st + 2] if st > 1 else [])
        out += [foreign[k % len(foreign)] for k in range(n_foreign)]
        return np.asarray(out, np.int64), max(max(out) + 1, lo + n_loc * st)

    uref, n_users = refs_of(users, urow, u_lo, u_st, n_ul, n_foreign_u)
    iref, n_items = refs_of(items, irow, i_lo, i_st, n_il, n_foreign_i)
    assert len(uref) == B and len(iref) == 2 * B, (name, d, len(uref), len(iref), B)
    rng = np.random.RandomState(1000 * d + CASE_NAMES.index(name))
    uref, iref = uref[rng.permutation(B)], iref[rng.permutation(2 * B)]
    stage = rng.randint(-STAGE_MAX, STAGE_MAX + 1, size=(3 * B, d)).astype(np.float32)
    want = [("u", p, L, tag) for L, tag, p in users if tag] + [("i", p, L, tag) for L, tag, p in items if tag]
    runs = [("u", p, L) for L, _, p in users] + [("i", p, L) for L, _, p in items]
    c = dict(runs=runs, d=d, name=name, B=B, n=3 * B, owned=owned, sharded=own is not None, n_users=n_users, n_items=n_items,
             u=uref.astype(np.int32), i=iref[:B].astype(np.int32), j=iref[B:].astype(np.int32), stage=stage, want=want)
    _cache[(d, name)] = c
    return c


# ---- what the kernels decide, restated ---------------------------------------------------------------------------------------
def _owned_local(row, lo, stride, n_loc):
    """owned_local of train_kernels.hip: the local index, or -1"""
    rel = row.astype(np.int64) - lo
    l = rel // stride
    return np.where((rel >= 0) & (l < n_loc) & (l * stride == rel), l, -1)


def ref_keys(c):
    """key of reference role * B + t, as k_shard_keys writes it (k_refs_init is the case every row is owned):
    user row -> local row, item row -> n_users_loc + local row, another rank's row -> key_end"""
    u_lo, u_st, n_ul, i_lo, i_st, n_il = c["owned"]
    none = n_ul + n_il
    lu = _owned_local(c["u"], u_lo, u_st, n_ul)
    li = _owned_local(np.concatenate([c["i"], c["j"]]), i_lo, i_st, n_il)
    return np.concatenate([np.where(lu >= 0, lu, none), np.where(li >= 0, n_ul + li, none)]).astype(np.int64)


def sorted_list(c):
    """the list the sort must produce: keys ascending, equal keys in reference order -> (sk, sv)"""
    if "_sorted" not in c:
        keys = ref_keys(c)
        sv = np.argsort(keys, kind="stable")
        c["_sorted"] = (keys[sv], sv)
    return c["_sorted"]


def layout(c):
    """One record per run of an owned row in the sorted list, in list order."""
    if "_layout" not in c:
        c["_layout"] = _layout(c)
    return c["_layout"]


def _layout(c):
    d, n = c["d"], c["n"]
    CH, R = ch_of(d), rpb_of(d)
    n_ul, n_il = c["owned"][2], c["owned"][5]
    key_end = n_ul + n_il
    sk, _ = sorted_list(c)
    nwin = (n + CH - 1) // CH
    first = np.flatnonzero((sk < key_end) & (np.concatenate([[-1], sk[:-1]]) != sk))
    ends = np.searchsorted(sk, sk[first], side="right")
    out = []
    for s, e in zip(first.tolist(), ends.tolist()):
        key, L = int(sk[s]), e - s
        rec = dict(key=key, table="u" if key < n_ul else "i", row=key if key < n_ul else key - n_ul, start=s, len=L, off=s % CH,
                   straddle=s // R != (e - 1) // R, last=e == n)
        # k_seg_reduce: heads at the first reference and at every multiple of CH; multi = the run leaves its first chunk
        heads = [s] + list(range((s // CH + 1) * CH, e, CH))
        rec["heads"] = heads
        rec["multi"] = len(heads) > 1
        rec["det_slots"] = [2 * (p // CH) + (p % CH != 0) for p in heads] if rec["multi"] else []
        # k_seg_fold: the windows behind the first that still start with the key, found by galloping + bisection
        w0 = s // CH
        starts = lambda w: sk[w * CH] == key                        # noqa: E731
        nc, hits = 0, False
        if w0 + 1 < nwin and starts(w0 + 1):
            lo, step = w0 + 1, 1
            while lo + step < nwin and starts(lo + step):
                lo += step
                step *= 2
            hi = lo + step if lo + step < nwin else nwin
            hits = hi == nwin
            while lo + 1 < hi:
                mid = (lo + hi) >> 1
                if starts(mid):
                    lo = mid
                else:
                    hi = mid
            nc = lo - w0
        rec["nc"], rec["fold_hits_nwin"] = nc, hits
        # k_seg_reduce_inv / k_seg_fold_inv: chunks from the run's start
        chunks = list(range(s, e, CH))
        rec["inv_heads"] = chunks
        rec["inv_multi"] = L > CH
        rec["inv_slots"] = [2 * (q // CH) + (q == s) for q in chunks] if L > CH else []
        inv_nc, inv_hits = 0, False
        if s + CH < n and sk[s + CH] == key:
            lo, step = s + CH, CH
            while lo + step < n and sk[lo + step] == key:
                lo += step
                step *= 2
            hi = lo + step if lo + step < n else n
            inv_hits = hi == n
            while lo + 1 < hi:
                mid = (lo + hi) >> 1
                if sk[mid] == key:
                    lo = mid
                else:
                    hi = mid
            inv_nc = (lo - s) // CH
        rec["inv_nc"], rec["inv_hits_n"] = inv_nc, inv_hits
        # k_seg_scan: a flag that names a run of <= 16, else flag 1 and one work item per 64 references
        lim = min(K_REF_RUN + 1, n - s)
        rec["scan_lim_cut"] = n - s < K_REF_RUN + 1
        ln = 1
        while ln < lim and sk[s + ln] == key:
            ln += 1
        if ln <= K_REF_RUN:
            rec["flag"], rec["work"], rec["scan_past_n"] = (ln << K_REF_SHIFT) | s, [], False
        else:
            lo, step = s + ln, K_REF_RUN
            while lo + step <= n and sk[lo + step - 1] == key:
                lo += step
                step *= 2
            rec["scan_past_n"] = lo + step > n
            hi = lo + step if lo + step < n else n
            while lo < hi:
                mid = (lo + hi) >> 1
                if sk[mid] == key:
                    lo = mid + 1
                else:
                    hi = mid
            total = lo - s
            rec["flag"] = 1
            rec["work"] = [(s + k * K_LONG_SPAN, min(K_LONG_SPAN, total - k * K_LONG_SPAN)) for k in range((total + K_LONG_SPAN - 1) // K_LONG_SPAN)]
        out.append(rec)
    return out


# ---- the integer model ---------------------------------------------------------------------------------------------------------
def row_sums(c, drop_ref=None):
    """int64 sums of the staging rows per owned row -> (SU[n_users_loc][d], SI[n_items_loc][d], refs per row cu, ci, max row
    sum of |terms|).  drop_ref: a reference left out (the sensitivity check)."""
    n_ul, n_il = c["owned"][2], c["owned"][5]
    keys = ref_keys(c)
    st = c["stage"].astype(np.int64)
    assert np.array_equal(st.astype(np.float32), c["stage"])
    keep = np.ones(c["n"], bool)
    if drop_ref is not None:
        keep[drop_ref] = False
    S = np.zeros((n_ul + n_il + 1, c["d"]), np.int64)
    A = np.zeros(n_ul + n_il + 1, np.int64)
    cnt = np.zeros(n_ul + n_il + 1, np.int64)
    np.add.at(S, keys[keep], st[keep])
    np.add.at(A, keys[keep], np.abs(st[keep]).max(axis=1))
    np.add.at(cnt, keys[keep], 1)
    return S[:n_ul], S[n_ul:n_ul + n_il], cnt[:n_ul], cnt[n_ul:n_ul + n_il], int(A[:n_ul + n_il].max(initial=0))


def initial(c, mode):
    """-> gU, gI (uint32 bit patterns, [n_loc + GUARD_ROWS][d]), tU, tI (int32 [n_loc + GUARD_ROWS]): NaN where the mode's kernels
    store, zero where they add atomically (REDUCE: the runs cut into chunks; INDEX: the runs of more than 16); None for a table
    without rows on this rank."""
    n_ul, n_il = c["owned"][2], c["owned"][5]
    g = {t: np.full((nl + GUARD_ROWS, c["d"]), NAN_BITS, np.uint32) for t, nl in (("u", n_ul), ("i", n_il))}
    for rec in layout(c):
        if (mode == "reduce" and rec["multi"]) or (mode == "index" and rec["len"] > K_REF_RUN):
            g[rec["table"]][rec["row"]] = 0
    f = {t: np.full(nl + GUARD_ROWS, FLAG_INIT, np.int32) for t, nl in (("u", n_ul), ("i", n_il))}
    return (g["u"] if n_ul else None, g["i"] if n_il else None, f["u"] if n_ul else None, f["i"] if n_il else None)


def expected(c, mode, drop_ref=None):
    """what the buffers of initial() must hold after the mode's launches, bit for bit"""
    SU, SI, cu, ci, _ = row_sums(c, drop_ref)
    gU, gI, tU, tI = (None if a is None else a.copy() for a in initial(c, mode))
    for g, t, S, cnt in ((gU, tU, SU, cu), (gI, tI, SI, ci)):
        if g is None:
            continue
        ref = np.flatnonzero(cnt > 0)
        if mode == "index":
            ref_long = np.flatnonzero(cnt > K_REF_RUN)
            g[ref_long] = S[ref_long].astype(np.float32).view(np.uint32)
        else:
            g[ref] = S[ref].astype(np.float32).view(np.uint32)
            t[ref] = 1
    if mode == "index":
        for rec in layout(c):
            (tU if rec["table"] == "u" else tI)[rec["row"]] = rec["flag"]
    return gU, gI, tU, tI


def compare(c, mode, got, want=None):
    """got = (gU, gI, tU, tI, sk, sv) as numpy (g as uint32 bit patterns); raises AssertionError naming the first wrong row"""
    want = expected(c, mode) if want is None else want
    sk, sv = sorted_list(c)
    assert np.array_equal(got[4].astype(np.int64), sk), "%s d=%d %s: sorted keys differ" % (c["name"], c["d"], mode)
    assert np.array_equal(got[5].astype(np.int64), sv), "%s d=%d %s: sorted values differ (the sort is not stable, or pairs split)" % (c["name"], c["d"], mode)
    by_row = {(r["table"], r["row"]): r for r in layout(c)}
    for tab, k in (("u", 0), ("i", 1)):
        g, w = got[k], want[k]
        if w is None:
            continue
        bad = np.flatnonzero((g != w).any(axis=1))
        if len(bad):
            r = int(bad[0])
            rec = by_row.get((tab, r))
            col = int(np.flatnonzero(g[r] != w[r])[0])
            raise AssertionError("%s d=%d %s: table %s row %d of %d (+%d guard rows) column %d: got %r want %r; %d rows differ; run: %r" % (
                c["name"], c["d"], mode, tab, r, len(w) - GUARD_ROWS, GUARD_ROWS, col, g[r, col:col + 1].view(np.float32)[0],
                w[r, col:col + 1].view(np.float32)[0], len(bad), rec))
        t, wt = got[2 + k], want[2 + k]
        badf = np.flatnonzero(t != wt)
        if len(badf):
            r = int(badf[0])
            raise AssertionError("%s d=%d %s: flag of table %s row %d: got 0x%x want 0x%x; %d flags differ; run: %r" % (
                c["name"], c["d"], mode, tab, r, int(t[r]) & 0xFFFFFFFF, int(wt[r]) & 0xFFFFFFFF, len(badf), by_row.get((tab, r))))
    if mode == "index":                       # a flag's run names exactly the row's references, in batch order
        keys = ref_keys(c)
        for rec in layout(c):
            if rec["len"] <= K_REF_RUN:
                pos, ln = rec["flag"] & ((1 << K_REF_SHIFT) - 1), rec["flag"] >> K_REF_SHIFT
                assert np.array_equal(got[5][pos:pos + ln].astype(np.int64), np.flatnonzero(keys == rec["key"])), rec


def upload(c, device="cuda"):
    """the case's batch and staging rows on the device (once per case: every mode reads the same)"""
    import torch
    return dict((k, torch.from_numpy(c[k]).to(device)) for k in ("u", "i", "j", "stage"))


def run_on_gpu(ops, c, mode, inputs, ws=None):
    """one call of macr_test_ref_reduce on the case's batch -> (got as compare() takes it, the workspace)"""
    import torch
    from macr_amd import _lib
    device = inputs["u"].device
    code = dict(reduce=_lib.TEST_REDUCE, index=_lib.TEST_INDEX, det=_lib.TEST_DET, inv=_lib.TEST_INV)[mode]
    if ws is None:
        ws = ops.test_ref_reduce_workspace(c["B"], c["d"], device)
        ws.fill_(0xFF)                                 # (all-ones words are NaN as floats: a slot read before it is written shows)
    dev = lambda a, dt: None if a is None else torch.from_numpy(a.view(dt)).to(device)      # noqa: E731
    ini = initial(c, mode)
    gU, gI = dev(ini[0], np.float32), dev(ini[1], np.float32)
    tU, tI = dev(ini[2], np.int32), dev(ini[3], np.int32)
    sk, sv = ops.test_ref_reduce(code, inputs["u"], inputs["i"], inputs["j"], inputs["stage"], c["owned"], gU, gI, tU, tI, ws)
    torch.cuda.synchronize()
    host = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)                     # noqa: E731
    return (host(gU, np.uint32), host(gI, np.uint32), host(tU, np.int32), host(tI, np.int32), host(sk, np.uint32), host(sv, np.uint32)), ws


def sensitivity_check(d=64, name="nc_big_inside"):
    """The comparison cannot pass vacuously: against a model that lost ONE reference of the hot row, the exact result fails.
    Host only: `got` is the exact result itself."""
    c = case(d, name)
    hot = max(layout(c), key=lambda r: r["len"])
    sk, sv = sorted_list(c)
    ref = int(sv[hot["start"] + hot["len"] // 2])
    assert np.any(c["stage"][ref] != 0)
    for mode in ("reduce", "det", "inv"):
        exact = expected(c, mode)
        got = exact + (sk.astype(np.uint32), sv.astype(np.uint32))
        compare(c, mode, got)                                   # the exact result passes ...
        lost = expected(c, mode, drop_ref=ref)
        try:
            compare(c, mode, got, want=lost)                    # ... and differs from the model that lost a reference
        except AssertionError as e:
            assert "row %d " % hot["row"] in str(e), str(e)
        else:
            raise AssertionError("a lost reference of a %d-reference row went unnoticed (%s)" % (hot["len"], mode))
    return hot["len"]
