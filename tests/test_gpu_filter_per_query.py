"""A row filter per query within one launch (include/mse.h "a filter per query").  The contract is parity: row i of an
_each call equals, bit for bit and counters included, the single-filter call made with query i alone and filters[i] -- the unfiltered call
where filters[i] is None.  So the existing calls, already pinned to the CPU oracle by tests/test_gpu_filtered_graph.py, are the
reference here; one test goes to the oracle directly."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_filtered_graph import K, LOWEST, N, NONE, SCALES, Index, clustered_rows

pytestmark = pytest.mark.gpu
COUNTERS = ("n_visited", "cmps", "pq_cmps")
NQ = 65                                  # more than one coalesced submission's 16, not a multiple of anything the kernels tile by


class Set:
    """An Index of tests/test_gpu_filtered_graph.py with what these tests add: 65 queries (f16, f32, tables), start nodes, an entry table
    on both graphs, and the filters the issue names -- among them three SHORTER than the graph (n_rows 31, 33, N - 1): their rows bound
    is what the per-query table carries next to the bitmap."""

    def __init__(self, mse, orc, d, seed):
        self.ix = ix = Index(mse, orc, d, seed)
        rng = np.random.default_rng(seed + 7)
        self.q32 = clustered_rows(orc, NQ, d, n_centres=48, seed=seed + 200).astype(np.float32)
        self.qh = orc.f16_bits(self.q32)
        self.luts = np.stack([ix.opq.preprocess_query(q) for q in orc.f16_to_f32(self.qh)])
        masks = {name: ix.masks[name] for name in ("half", "tenth", "pct", "all", "none")}
        for n_rows in (31, 33, N - 1):
            m = rng.random(n_rows) < 0.5
            m[5] = True                                              # row 5 is allowed by every short filter (a start node below)
            masks["short%d" % n_rows] = m
        self.masks = masks
        self.filters = {name: (ix.filters[name] if name in ix.filters else mse.RowFilter(m)) for name, m in masks.items()}
        self.names = ["half", "tenth", "pct", "all", "none", None, "short31", "short33", "short%d" % (N - 1)]
        self.per_query = [self.names[i % len(self.names)] for i in range(NQ)]
        self.starts = rng.integers(0, N, size=NQ).astype(np.uint32)
        for i, name in enumerate(self.per_query):
            if name in ("short31", "short33"):
                self.starts[i] = 5                                   # fetched first: the only way a search meets rows 0 .. 32
        self.entry_ids = np.sort(rng.choice(N, 40, replace=False)).astype(np.uint32)
        for g in ix.graphs.values():
            mse.set_entries(g, ix.vecs, self.entry_ids)

    def flts(self, names):
        return [self.filters[n] if n is not None else None for n in names]


@pytest.fixture(scope="module")
def small(gpu, mse, orc):
    return Set(mse, orc, 128, 41)


@pytest.fixture(scope="module")
def big(gpu, mse, orc):
    return Set(mse, orc, 1152, 42)


def same(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    for c in COUNTERS:
        assert np.array_equal(a[2][c], b[2][c]), (what, c)


def stack(rows):
    """one-query answers as the [nq, k] answer of a batch"""
    return (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]),
            {c: np.concatenate([r[2][c] for r in rows]) for c in COUNTERS})


def cut(res, idx):
    return res[0][idx], res[1][idx], {c: res[2][c][idx] for c in COUNTERS}


def topk(mse, st, searcher, g, idx, f32, use_scales, use_starts, disable_pq, beam, L, **kw):
    """disk_query_topk over the queries `idx` of the set"""
    idx = np.asarray(idx)
    q = st.q32[idx] if f32 else st.qh[idx]
    luts = None if f32 or disable_pq else st.luts[idx]
    return mse.disk_query_topk(searcher, st.ix.gpq, st.ix.gcodes, g, q, K, st.starts[idx] if use_starts else None, luts,
                               SCALES if use_scales else None, disable_pq, beam, L, **kw)


def lone_calls(mse, st, searcher, g, idx, names, *args, regime="graph", **kw):
    rows = []
    for i, name in zip(idx, names):
        fkw = dict(filter=st.filters[name], regime=regime) if name is not None else {}
        rows.append(topk(mse, st, searcher, g, [i], *args, **fkw, **kw))
    return stack(rows)


# (disable_pq, beam, search_list): the ADC kernel, the exact kernel at a short list with a small beam, the exact kernel past 256 entries
CONFIGS = {"adc": (False, 4, 48), "exact": (True, 2, 48), "exact_long": (True, 2, 300)}


@pytest.mark.parametrize("with_url", [False, True])
@pytest.mark.parametrize("use_starts", [True, False])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_each_call_equals_the_lone_calls(small, mse, config, use_starts, with_url):
    """nq in {1, 2, 65}, a different filter per query -- half, tenth, percent, all, none, NULL, and three filters shorter than the graph --
    against the concatenation of the one-query single-filter calls: ids, scores and the three counters.  ADC and exact scoring, a list
    below and above 256; a graph with and without a has_url array; start nodes given and by the entry table; f16 and f32 queries;
    descriptor scales on and off."""
    st = small
    g = st.ix.graphs[with_url]
    disable_pq, beam, L = CONFIGS[config]
    for f32 in (False, True):
        for use_scales in (True, False):
            args = (f32, use_scales, use_starts, disable_pq, beam, L)
            want = lone_calls(mse, st, st.ix.searcher, g, range(NQ), st.per_query, *args)
            for nq in (1, 2, NQ):
                got = topk(mse, st, st.ix.searcher, g, range(nq), *args, filter=st.flts(st.per_query[:nq]), regime="graph")
                same(got, cut(want, slice(0, nq)), (config, f32, use_scales, nq))
            # the answers are not degenerate: the dense filters fill their k, the empty one returns padding, the short ones stay below
            # their bound (and -- start nodes given, no has_url array to veto row 5 -- are not empty)
            for i, name in enumerate(st.per_query):
                if name in ("half", "all", None):
                    assert np.all(want[0][i] != NONE), (name, i)
                if name == "none":
                    assert np.all(want[0][i] == NONE) and np.all(want[1][i] == LOWEST) and want[2]["n_visited"][i] == 0
                    assert want[2]["cmps"][i] > 0                         # explicit GRAPH still traverses
                if name in ("short31", "short33"):
                    live = want[0][i][want[0][i] != NONE]
                    assert np.all(live < int(name[5:]))
                    assert not (use_starts and not with_url) or 5 in live


@pytest.mark.parametrize("disable_pq", [False, True])
def test_each_call_equals_the_lone_calls_at_full_width(big, mse, disable_pq):
    """the same at 1152 dimensions, both scoring kinds, f16 queries with tables and f32 queries"""
    st = big
    g = st.ix.graphs[True]
    for f32 in (False, True):
        args = (f32, True, True, disable_pq, 4, 64)
        want = lone_calls(mse, st, st.ix.searcher, g, range(NQ), st.per_query, *args)
        got = topk(mse, st, st.ix.searcher, g, range(NQ), *args, filter=st.flts(st.per_query), regime="graph")
        same(got, want, (disable_pq, f32))
        assert np.all(want[0][0] != NONE)


def test_one_wave_kernel_reads_the_table(small, mse):
    """More than 1024 exactly scored queries at a list and pre-buffer of at most 256 run one wave per query: 1100 queries, each with one
    of nine filters, against the single-filter batch calls over each filter's queries and -- every ninth query -- the lone call."""
    st = small
    g = st.ix.graphs[True]
    nq = 1100
    idx = np.arange(nq) % NQ
    names = [st.names[(i * 4) % len(st.names)] for i in range(nq)]       # (4 and 9 are coprime: every query meets every filter)
    args = (False, True, True, True, 3, 40)
    got = topk(mse, st, st.ix.searcher, g, idx, *args, filter=st.flts(names), regime="graph")
    for name in st.names:
        rows = np.array([i for i in range(nq) if names[i] == name])
        fkw = dict(filter=st.filters[name], regime="graph") if name is not None else {}
        same(cut(got, rows), topk(mse, st, st.ix.searcher, g, idx[rows], *args, **fkw), name)
    sample = list(range(0, nq, 9))
    same(cut(got, sample), lone_calls(mse, st, st.ix.searcher, g, idx[sample], [names[i] for i in sample], *args), "lone")


@pytest.mark.parametrize("which", ["exact", "adc"])
def test_list_form_against_the_oracle(small, big, mse, orc, which):
    """disk_search_batch(filter=[...]) against orc.disk_greedy_search over has_url AND mask_i, query by query: the search list, the
    visited list in fetch order and the counters."""
    st, disable_pq, beam, L, scales = (small, True, 2, 40, None) if which == "exact" else (big, False, 4, 48, SCALES)
    ix = st.ix
    names = [st.names[i % len(st.names)] for i in range(ix.nq)]
    for with_url in (True, False):
        got = mse.disk_search_batch(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.starts, ix.qh, ix.luts, scales, disable_pq, beam,
                                    search_list=L, visited_cap=N, filter=st.flts(names))
        filled = 0
        for i, name in enumerate(names):
            allowed = np.ones(N, bool)
            if name is not None:
                allowed[:] = False
                allowed[:len(st.masks[name])] = st.masks[name]
            url = (allowed & (ix.has_url.astype(bool) if with_url else True)).astype(np.uint8)
            obuf, ovids, ovsc, ocm, opc = ix.oracle(orc, i, L, beam, disable_pq, scales, url)
            bi, bs, vi, vs, cm, pc = got[i]
            assert (cm, pc) == (ocm, opc), (name, i)
            assert np.array_equal(bi, obuf.ids) and np.array_equal(bs, obuf.scores), (name, i)
            assert np.array_equal(vi, ovids) and np.array_equal(vs, ovsc), (name, i)
            filled += len(ovids)
        assert filled > 0


def test_auto_resolves_every_query_on_its_own(small, mse):
    """AUTO over filters whose plans differ -- GRAPH at L, GRAPH at a widened L', LIST, empty, unfiltered -- equals the explicit one-query
    calls at mse.filtered_plan's answers, in the caller's order; and explicit LIST with two filter objects interleaved equals the
    per-filter LIST calls."""
    st = small
    ix = st.ix
    g = ix.graphs[True]
    L = 200
    rng = np.random.default_rng(3)
    wide = mse.RowFilter(rng.choice(N, 3907, replace=False), n_rows=N)       # L' = 1024
    pool = [("all", st.filters["all"]), ("half", st.filters["half"]), ("wide", wide), ("pct", st.filters["pct"]), ("none", st.filters["none"]),
            (None, None)]
    plans = {name: (mse.filtered_plan(N, f.count, L) if f is not None else ("graph", L)) for name, f in pool}
    assert plans["all"] == ("graph", L) and plans["half"][0] == "graph" and L < plans["half"][1] < 1024
    assert plans["wide"] == ("graph", 1024) and plans["pct"] == ("list", L) and plans["none"] == ("list", L)
    nq = 20
    per = [pool[(i * 5) % len(pool)] for i in range(nq)]                      # interleaved: every class is scattered over the call
    args = (False, True, True, False, 4)
    got = topk(mse, st, ix.searcher, g, range(nq), *args, L, filter=[f for _, f in per], regime="auto")
    rows = []
    for i, (name, f) in enumerate(per):
        regime, eff = plans[name]
        fkw = dict(filter=f, regime=regime) if f is not None else {}
        rows.append(topk(mse, st, ix.searcher, g, [i], *args, eff, **fkw))
    same(got, stack(rows), "auto")
    for i, (name, _) in enumerate(per):
        if name == "pct":
            assert got[2]["pq_cmps"][i] == 0 and got[2]["cmps"][i] == got[2]["n_visited"][i] > 0
        elif name == "none":
            assert got[2]["cmps"][i] == 0 and np.all(got[0][i] == NONE)
        else:
            assert got[2]["pq_cmps"][i] > 0
    # the same call with the f16 queries already on the device: the classes are gathered from one fetched copy
    import torch
    qd = torch.from_numpy(st.qh[:nq].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    on_dev = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, (qd.data_ptr(), nq), K, st.starts[:nq], st.luts[:nq], SCALES, False, 4, L,
                                 filter=[f for _, f in per], regime="auto")
    same(on_dev, got, "device-resident queries")
    # explicit LIST, two filter objects interleaved
    two = [st.filters["pct"], ix.filters["few"]]
    got = topk(mse, st, ix.searcher, g, range(nq), *args, L, filter=[two[i % 2] for i in range(nq)], regime="list")
    for j, f in enumerate(two):
        rows = np.arange(j, nq, 2)
        same(cut(got, rows), topk(mse, st, ix.searcher, g, rows, *args, L, filter=f, regime="list"), ("list", j))


def test_with_the_de_duplication_and_with_a_grouping(small, mse):
    """mse_graph_set_dedup on, GRAPH regime: equal to the lone calls; with groups=: equal to the grouped lone calls."""
    st = small
    ix = st.ix
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    # vectors of its own: a tenth of the rows are copies of their nearest neighbour, so that the de-duplication has something to remove
    rng = np.random.default_rng(8)
    base = ix.base.copy()
    dst = rng.choice(N, N // 10, replace=False)
    base[dst] = ix.base[ix.adj[dst, 0]]
    vecs = mse.VectorList.from_f16s(base, ix.d)
    s = mse.Searcher(vecs)
    nq = 33
    args = (False, True, True, False, 4, 64)
    flts = st.flts(st.per_query[:nq])
    mse.set_dedup(g, 0.95)
    want = lone_calls(mse, st, s, g, range(nq), st.per_query[:nq], *args)
    same(topk(mse, st, s, g, range(nq), *args, filter=flts, regime="graph"), want, "dedup")
    mse.set_dedup(g, 0.0)
    plain = lone_calls(mse, st, s, g, range(nq), st.per_query[:nq], *args)
    assert any(not np.array_equal(want[0][i], plain[0][i]) for i in range(nq))      # the de-duplication did remove something
    groups = mse.RowGroups(rng.integers(0, 50, size=N).astype(np.uint32))
    rows = []
    for i, name in enumerate(st.per_query[:nq]):
        rows.append(topk(mse, st, s, g, [i], *args, groups=groups, filter=st.filters[name] if name is not None else None, regime="graph"))
    want = stack(rows)
    same(topk(mse, st, s, g, range(nq), *args, filter=flts, regime="graph", groups=groups), want, "groups")
    assert any(not np.array_equal(want[0][i], plain[0][i]) for i in range(nq))


def test_uniform_launches_are_the_single_filter_launches(small, mse):
    """The same filter object nq times equals the single-filter batch call; all None equals the unfiltered call."""
    st = small
    g = st.ix.graphs[True]
    for disable_pq in (False, True):
        args = (False, True, False, disable_pq, 4, 48)
        f = st.filters["half"]
        same(topk(mse, st, st.ix.searcher, g, range(NQ), *args, filter=[f] * NQ, regime="graph"),
             topk(mse, st, st.ix.searcher, g, range(NQ), *args, filter=f, regime="graph"), "one object")
        same(topk(mse, st, st.ix.searcher, g, range(NQ), *args, filter=[None] * NQ), topk(mse, st, st.ix.searcher, g, range(NQ), *args), "all None")


def test_distinct_filters_share_submissions(small, mse):
    """64 threads behind a barrier, each making one-query GRAPH calls with its OWN filter object at one search_list, unfiltered callers
    among them: every answer is the lone call's, and they SHARED LAUNCHES.  The coalescer gathers waiting requests into batches
    (coalescer_stats: passes) whatever their filters and then splits each batch into groups that can share a launch
    (coalescer_groups) -- the split is what the sharing rule decides.  Here every batch must stay ONE group (groups == passes, fewer
    than requests); before the launch read a filter per query every distinct filter object was a group of its own.  The same for 64
    tickets from one thread; and the control: LIST requests with distinct filter objects must NOT share (groups == requests)."""
    st = small
    ix = st.ix
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    mse.set_entries(g, ix.vecs, st.entry_ids)
    T, L, beam, rounds = 64, 48, 4, 3
    rng = np.random.default_rng(21)
    own = [None if i % 8 == 7 else mse.RowFilter(rng.random(N) < (0.5 if i % 2 else 0.1)) for i in range(T)]
    lone = mse.Searcher(ix.vecs)

    def call(s, i):
        fkw = dict(filter=own[i], regime="graph") if own[i] is not None else {}
        return mse.disk_query_topk(s, ix.gpq, ix.gcodes, g, st.q32[i:i + 1], K, None, None, SCALES, False, beam, L, **fkw)

    want = [call(lone, i) for i in range(T)]
    assert all(np.any(w[0] != NONE) for w in want)
    got, errs = [None] * T, []
    gate = threading.Barrier(T)

    def worker(i):
        try:
            gate.wait()
            for _ in range(rounds):
                got[i] = call(ix.searcher, i)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    def counters():
        st, gr = mse.coalescer_stats(g), mse.coalescer_groups(g)
        return np.array([st["requests"], st["passes"], gr["groups"], gr["requests"]], np.int64)

    before = counters()
    th = [threading.Thread(target=worker, args=(i,)) for i in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(T):
        same(got[i], want[i], i)
    requests, passes, groups, grouped = counters() - before
    print(f"threads: {requests} requests, {passes} batches, {groups} launch groups")
    assert requests == grouped == rounds * T
    assert groups == passes < requests                # no batch was split by filter object, and batches held several requests
    # tickets: one object, one thread, a filter per request
    tk = mse.QueryTickets(ix.searcher, ix.gpq, ix.gcodes, g, K, False, beam, L, regime="graph")
    before = counters()
    for i in range(T):
        tk.submit(st.q32[i], SCALES, key=i, filter=own[i])
    done = {}
    while len(done) < T:
        back = tk.collect(timeout_us=5_000_000)
        assert back, "no ticket came back within five seconds"
        for key, ids, sc in back:
            done[key] = (ids, sc)
    for i in range(T):
        assert np.array_equal(done[i][0], want[i][0]) and np.array_equal(done[i][1], want[i][1]), i
    requests, passes, groups, grouped = counters() - before
    print(f"tickets: {requests} requests, {passes} batches, {groups} launch groups")
    assert requests == grouped == T and groups == passes < T
    # the control: a list pass serves ONE filter object, so LIST requests with a filter object each never share a launch
    small_own = [mse.RowFilter(rng.choice(N, 50, replace=False), n_rows=N) for _ in range(T)]
    tk = mse.QueryTickets(ix.searcher, ix.gpq, ix.gcodes, g, K, False, beam, L, regime="list")
    want_list = [mse.disk_query_topk(lone, ix.gpq, ix.gcodes, g, st.q32[i:i + 1], K, None, None, SCALES, False, beam, L, filter=small_own[i],
                                     regime="list") for i in range(T)]
    before = counters()
    for i in range(T):
        tk.submit(st.q32[i], SCALES, key=i, filter=small_own[i])
    done = {}
    while len(done) < T:
        back = tk.collect(timeout_us=5_000_000)
        assert back, "no ticket came back within five seconds"
        for key, ids, sc in back:
            done[key] = (ids, sc)
    for i in range(T):
        assert np.array_equal(done[i][0], want_list[i][0]) and np.array_equal(done[i][1], want_list[i][1]), i
    requests, passes, groups, grouped = counters() - before
    print(f"LIST tickets: {requests} requests, {passes} batches, {groups} launch groups")
    assert requests == grouped == groups == T and passes <= T


def test_a_long_lived_handle_answers_as_a_fresh_one(small, mse):
    """One Searcher through: an _each call of many queries, an unfiltered call, a single-filter call, an _each call of one query, an
    _each call with other filters -- each answer equals that of a handle made for it alone."""
    st = small
    ix = st.ix
    g = ix.graphs[True]
    args = (False, True, True, False, 4, 48)
    other = st.per_query[3:] + st.per_query[:3]
    steps = [lambda s: topk(mse, st, s, g, range(NQ), *args, filter=st.flts(st.per_query), regime="auto"),
             lambda s: topk(mse, st, s, g, range(20), *args),
             lambda s: topk(mse, st, s, g, range(20), *args, filter=st.filters["tenth"], regime="graph"),
             lambda s: topk(mse, st, s, g, [4], *args, filter=st.flts(st.per_query[4:5]), regime="graph"),
             lambda s: topk(mse, st, s, g, range(NQ), *args, filter=st.flts(other), regime="graph")]
    old = mse.Searcher(ix.vecs)
    for n, step in enumerate(steps):
        same(step(old), step(mse.Searcher(ix.vecs)), n)


def test_errors_name_the_query_and_write_nothing(small, mse):
    """A null array, an over-long filter at position 3 of 5, an unknown regime, LIST under the de-duplication: non-zero, the single-filter
    call's message -- with the query's position where an entry is at fault -- and outputs prefilled with a sentinel untouched."""
    from mse import ffi
    st = small
    ix = st.ix
    lib = ffi.lib()
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    too_long = mse.RowFilter(np.ones(N + 1, bool))
    ok, pct = st.filters["half"], st.filters["pct"]
    u32, i64, u16, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    nq = 5
    q16, q32 = np.ascontiguousarray(st.qh[:nq]), np.ascontiguousarray(st.q32[:nq])
    starts = np.ascontiguousarray(st.starts[:nq])

    def arr(*fs):
        return (C.c_void_p * nq)(*[f._h if f is not None else None for f in fs])

    cases = [(None, 1, "null filters array", None),
             (arr(ok, None, ok, too_long, ok), 1, "longer", 3),
             (arr(ok, ok, None, ok, ok), 7, "regime", None),
             (arr(ok, pct, ok, pct, None), 2, "de-duplicate", 0)]
    mse.set_dedup(g, 0.95)
    for filters, regime, word, at in cases:
        oi, os_, cnt = np.full((nq, K), 123, np.uint32), np.full((nq, K), 456, np.int64), np.full((3, nq), 789, np.uint32)
        outs = (oi.ctypes.data_as(u32), os_.ctypes.data_as(i64), cnt[0].ctypes.data_as(u32), cnt[1].ctypes.data_as(u32), cnt[2].ctypes.data_as(u32))
        head = (ix.searcher._h, None, None, g._h, filters, regime, None, starts.ctypes.data_as(u32))
        assert lib.mse_disk_query_topk_filtered_each(*head, q16.ctypes.data_as(u16), None, None, nq, 1, 4, 50, K, *outs) != 0
        msg = ffi.last_error()
        assert word in msg and (at is None or "(query %d)" % at in msg), msg
        assert lib.mse_disk_query_topk_filtered_each_f32(*head, q32.ctypes.data_as(f32p), None, nq, 1, 4, 50, K, *outs) != 0
        msg = ffi.last_error()
        assert word in msg and (at is None or "(query %d)" % at in msg), msg
        assert np.all(oi == 123) and np.all(os_ == 456) and np.all(cnt == 789), word
        if regime == 1:                                                    # the list form is GRAPH only
            bi, bs, bl = np.full((nq, 50), 123, np.uint32), np.full((nq, 50), 456, np.int64), np.full(nq, 789, np.uint32)
            assert lib.mse_disk_search_batch_filtered_each(ix.searcher._h, None, None, g._h, filters, starts.ctypes.data_as(u32), q16.ctypes.data_as(u16),
                                                           None, None, nq, 1, 4, 50, bi.ctypes.data_as(u32), bs.ctypes.data_as(i64), bl.ctypes.data_as(u32),
                                                           None, None, 0, *outs[2:]) != 0
            msg = ffi.last_error()
            assert word in msg and (at is None or "(query %d)" % at in msg), msg
            assert np.all(bi == 123) and np.all(bs == 456) and np.all(bl == 789) and np.all(cnt == 789)
    # a call of several classes (AUTO: the percent filter scans, the half filter traverses) whose LAST class has a start node out of
    # range: found before the first class runs, so nothing is written
    mse.set_dedup(g, 0.0)
    bad = starts.copy()
    bad[4] = N + 5
    oi, os_, cnt = np.full((nq, K), 123, np.uint32), np.full((nq, K), 456, np.int64), np.full((3, nq), 789, np.uint32)
    outs = (oi.ctypes.data_as(u32), os_.ctypes.data_as(i64), cnt[0].ctypes.data_as(u32), cnt[1].ctypes.data_as(u32), cnt[2].ctypes.data_as(u32))
    assert mse.filtered_plan(N, pct.count, 50)[0] == "list" and mse.filtered_plan(N, ok.count, 50)[0] == "graph"
    assert lib.mse_disk_query_topk_filtered_each(ix.searcher._h, None, None, g._h, arr(pct, ok, pct, ok, ok), 0, None, bad.ctypes.data_as(u32),
                                                 q16.ctypes.data_as(u16), None, None, nq, 1, 4, 50, K, *outs) != 0
    assert "start node" in ffi.last_error(), ffi.last_error()
    assert np.all(oi == 123) and np.all(os_ == 456) and np.all(cnt == 789)
    mse.set_dedup(g, 0.95)
    # LIST under the de-duplication is fine for a filter that allows nothing, as in the single-filter call
    got = topk(mse, st, ix.searcher, g, range(2), False, False, True, True, 4, 50, filter=[st.filters["none"]] * 2, regime="list")
    assert np.all(got[0] == NONE) and np.all(got[2]["cmps"] == 0)
    with pytest.raises(mse.MseError, match="filters for"):
        topk(mse, st, ix.searcher, g, range(3), False, False, True, True, 4, 50, filter=[ok, ok], regime="graph")
