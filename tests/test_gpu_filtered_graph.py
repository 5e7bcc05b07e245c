"""Filtered graph search against the CPU oracle, bit for bit.  A filtered search is the reference's greedy_search over an index whose
has_url is (has_url AND allowed) (src/query_disk_index.rs:172), so the existing oracle defines every output of the GRAPH regime; the
LIST regime is orc.score_all + orc.descriptor_product + a sort over the eligible rows; AUTO is the explicit call at mse_filtered_plan's
answer."""
import threading

import numpy as np
import pytest

from conftest import SEED_CENTRES

pytestmark = pytest.mark.gpu
N, K = 20000, 10
NONE, LOWEST = 0xFFFFFFFF, np.iinfo(np.int64).min
SCALES = np.array([0.5, 0, -0.25, 1.0], np.float32) / np.float32(512)


# ---- fixtures as tests/test_gpu_pq_index_graph.py builds them (helpers copied; the width is a parameter here) --------------------------
def clustered_rows(orc, n, d, n_centres=64, noise=0.3, seed=0):
    """Unit rows around `n_centres` unit centres (iid Gaussian data is not quantisable)."""
    rng = np.random.default_rng(seed)
    centres = orc.f16_to_f32(orc.gen_rows_f16(SEED_CENTRES, 0, n_centres))[:, :d]
    centres = centres / np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[rng.integers(0, n_centres, n)] + rng.standard_normal((n, d)).astype(np.float32) * np.float32(noise / np.sqrt(d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def train_pq(orc, sample, dpc, n_centroids=256, iters=2, seed=1):
    """Tiny OPQ-shaped codec: random orthonormal transform, per-subspace max-inner-product k-means."""
    rng = np.random.default_rng(seed)
    d = sample.shape[1]
    T = np.linalg.qr(rng.standard_normal((d, d)))[0].astype(np.float32)
    t = sample @ T.T
    cents = np.zeros((n_centroids, d), np.float32)
    for i in range(d // dpc):
        sub = t[:, i * dpc:(i + 1) * dpc]
        c = sub[rng.choice(len(sub), n_centroids, replace=False)].copy()
        for _ in range(iters):
            a = np.argmax(sub @ c.T, axis=1)
            for j in range(n_centroids):
                m = sub[a == j]
                if len(m):
                    c[j] = m.mean(axis=0)
        cents[:, i * dpc:(i + 1) * dpc] = c
    return cents, T


def knn_graph(x, deg, rng, long_edges=4):
    """Small navigable graph: nearest neighbours by dot product + a few random edges (in row blocks: n x n floats are not held)."""
    n = len(x)
    near = np.empty((n, deg - long_edges), np.int64)
    for r0 in range(0, n, 2000):
        s = x[r0:r0 + 2000] @ x.T
        s[np.arange(s.shape[0]), r0 + np.arange(s.shape[0])] = -np.inf
        part = np.argpartition(-s, deg - long_edges, axis=1)[:, :deg - long_edges]
        order = np.argsort(-np.take_along_axis(s, part, axis=1), axis=1, kind="stable")
        near[r0:r0 + 2000] = np.take_along_axis(part, order, axis=1)
    adj = np.concatenate([near, rng.integers(0, n, size=(n, long_edges))], axis=1).astype(np.uint32)
    degs = rng.integers(deg - 2, deg + 1, size=n).astype(np.uint32)
    return adj, degs


class Index:
    """One index of N rows at width d: rows, codec, codes, descriptors, graph (with and without a has_url array), queries, and the
    filters the issue names."""

    def __init__(self, mse, orc, d, seed):
        rng = np.random.default_rng(seed)
        self.d, self.n = d, N
        self.x = clustered_rows(orc, N, d, n_centres=48, seed=seed)
        self.base = orc.f16_bits(self.x)
        cents, T = train_pq(orc, self.x[:1500], d // 64)
        self.opq, self.gpq = orc.PQ(cents, T, d // 64, d), mse.ProductQuantizer(cents, T, d // 64, d)
        t = orc.f16_to_f32(self.base) @ T.T                               # codes by numpy (any code bytes are an index; these are good ones)
        dpc = d // 64
        self.codes = np.stack([np.argmax(t[:, i * dpc:(i + 1) * dpc] @ cents[:, i * dpc:(i + 1) * dpc].T, axis=1) for i in range(64)],
                              axis=1).astype(np.uint8)
        self.desc = rng.integers(0, 256, size=(N, 4), dtype=np.uint8)
        self.adj, self.degs = knn_graph(self.x, 16, rng)
        self.has_url = (rng.random(N) > 0.1).astype(np.uint8)
        self.starts = rng.integers(0, N, size=12).astype(np.uint32)
        self.has_url[self.starts[:2]] = 1
        self.vecs = mse.VectorList.from_f16s(self.base, d)
        self.searcher = mse.Searcher(self.vecs)
        self.gcodes = mse.Codes(self.codes, self.desc)
        self.graphs = {True: mse.DeviceGraph(mse.IndexGraph(self.adj, self.degs), self.has_url),
                       False: mse.DeviceGraph(mse.IndexGraph(self.adj, self.degs))}
        self.nq = 12
        self.qs = clustered_rows(orc, self.nq, d, n_centres=48, seed=seed + 100)
        self.qh = orc.f16_bits(self.qs)
        self.luts = np.stack([self.opq.preprocess_query(q) for q in orc.f16_to_f32(self.qh)])
        masks = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "half": rng.random(N) < 0.5, "tenth": rng.random(N) < 0.1}
        one = np.zeros(N, bool)
        one[self.starts[0]] = True                                      # the first query's start node: fetched first, and it has a url
        few = np.zeros(N, bool)
        few[rng.choice(N, K - 3, replace=False)] = True                 # fewer than k
        pct = np.zeros(N, bool)
        pct[rng.choice(N, 199, replace=False)] = True                   # 1 %: random rows and the second query's start node
        pct[self.starts[1]] = True
        short = rng.random(N - 3333) < 0.5                              # a filter shorter than the graph: the rows past it are excluded
        masks.update(one=one, few=few, pct=pct, short=short)
        self.masks = masks
        self.filters = {name: mse.RowFilter(m) for name, m in masks.items()}

    def allowed(self, name):
        m = np.zeros(self.n, bool)
        m[:len(self.masks[name])] = self.masks[name]
        return m

    def eff_url(self, name, with_url):
        """has_url AND allowed: the has_url array of the index the oracle searches"""
        return (self.allowed(name) & (self.has_url.astype(bool) if with_url else True)).astype(np.uint8)

    def oracle(self, orc, i, L, beam, disable_pq, scales, url, start=None, qh=None, lut=None):
        return orc.disk_greedy_search(self.base, self.adj, self.degs, self.codes, self.desc, int(self.starts[i] if start is None else start),
                                      self.qh[i] if qh is None else qh, self.luts[i] if lut is None else lut, scales, disable_pq, beam, L, url)


@pytest.fixture(scope="module")
def big(gpu, mse, orc):
    return Index(mse, orc, 1152, 31)


@pytest.fixture(scope="module")
def small(gpu, mse, orc):
    return Index(mse, orc, 128, 32)


def sorted_cut(ids, sc, k):
    """the request path's last step: (score desc, id asc), first k, padded"""
    order = sorted(range(len(ids)), key=lambda j: (-int(sc[j]), int(ids[j])))[:k]
    wi, ws = np.full(k, NONE, np.uint32), np.full(k, LOWEST, np.int64)
    wi[:len(order)] = np.asarray(ids, np.uint32)[order]
    ws[:len(order)] = np.asarray(sc, np.int64)[order]
    return wi, ws


def check_list_form(ix, orc, got, L, beam, disable_pq, scales, url, queries):
    filled = 0
    for i in queries:
        obuf, ovids, ovsc, ocm, opc = ix.oracle(orc, i, L, beam, disable_pq, scales, url)
        bi, bs, vi, vs, cm, pc = got[i]
        assert (cm, pc) == (ocm, opc), i
        assert np.array_equal(bi, obuf.ids) and np.array_equal(bs, obuf.scores), i
        assert np.array_equal(vi, ovids) and np.array_equal(vs, ovsc), i
        filled += len(ovids)
    return filled


FILTER_NAMES = ["none", "one", "few", "pct", "tenth", "half", "all", "short"]
GRID = [(b, dp, sc, L) for b in (1, 4, 8) for dp in (False, True) for sc in (True, False) for L in (12, 200, 1024)]


@pytest.mark.parametrize("beam,disable_pq,use_scales,L", GRID)
def test_filtered_list_form_matches_oracle_over_the_parameter_range(big, mse, orc, beam, disable_pq, use_scales, L):
    """mse_disk_search_batch_filtered: search lists, visited lists in fetch order and the three counters equal the oracle's search over
    has_url AND allowed, for beamwidth {1, 4, 8} x {ADC, disable_pq} x {scales, none} x L {12, 200, 1024}; the filter and the kind of
    graph (with / without a has_url array) rotate through the grid so that each meets every parameter value."""
    ix = big
    case = GRID.index((beam, disable_pq, use_scales, L))
    name = FILTER_NAMES[case % len(FILTER_NAMES)]
    with_url = bool((case // len(FILTER_NAMES) + case) % 2)
    scales = SCALES if use_scales else None
    nq = 6 if L == 1024 else ix.nq
    got = mse.disk_search_batch(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.starts[:nq], ix.qh[:nq], ix.luts[:nq], scales,
                                disable_pq, beam, search_list=L, visited_cap=N, filter=ix.filters[name])
    filled = check_list_form(ix, orc, got, L, beam, disable_pq, scales, ix.eff_url(name, with_url), range(nq))
    print(f"filter {name}, has_url array {with_url}: {filled} visited records over {nq} queries")
    assert filled == 0 if name == "none" else filled > 0 or name in ("few", "pct")


@pytest.mark.parametrize("name", FILTER_NAMES)
@pytest.mark.parametrize("with_url", [False, True])
def test_every_filter_on_both_kinds_of_graph(big, small, mse, orc, name, with_url):
    """Each filter of the issue's list -- none allowed, one row, fewer than k, 1 %, 10 %, 50 %, all, shorter than the graph -- on a graph
    with and without a has_url array, at d = 1152 (ADC, beam 4) and d = 128 (exact, beam 2): list form and request path (explicit
    GRAPH), padding included.  Non-degeneracy: for 50 % and 10 % L is picked on the CPU so that the ORACLE's filtered visited list
    holds at least k records for every query; for the sparse filters only that the oracle's lists are not all empty."""
    for ix, beam, disable_pq, scales in ((big, 4, False, SCALES), (small, 2, True, None)):
        url = ix.eff_url(name, with_url)
        L = 48
        if name in ("half", "tenth"):
            for L in (12, 24, 48, 100, 200, 400, 1024):
                if all(len(ix.oracle(orc, i, L, beam, disable_pq, scales, url)[1]) >= K for i in range(ix.nq)):
                    break
            else:
                pytest.fail("no search_list gives every query k allowed visited records")
        g = ix.graphs[with_url]
        got = mse.disk_search_batch(ix.searcher, ix.gpq, ix.gcodes, g, ix.starts, ix.qh, ix.luts, scales, disable_pq, beam, search_list=L,
                                    visited_cap=N, filter=ix.filters[name])
        filled = check_list_form(ix, orc, got, L, beam, disable_pq, scales, url, range(ix.nq))
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, scales, disable_pq, beam, L,
                                          filter=ix.filters[name], regime="graph")
        for i in range(ix.nq):
            _, ovids, ovsc, ocm, opc = ix.oracle(orc, i, L, beam, disable_pq, scales, url)
            wi, ws = sorted_cut(ovids, ovsc, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (name, i)
            assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (ocm, opc, len(ovids)), (name, i)
            if name in ("half", "tenth", "all"):
                assert len(ovids) >= K and np.all(ids[i] != NONE)
        if name == "none":
            assert filled == 0 and np.all(ids == NONE) and np.all(sc == LOWEST)
        elif name in ("pct", "few", "one", "short"):
            assert name == "few" or filled > 0                            # (K - 3 random rows of 20 000 may honestly never be fetched)
            assert name != "short" or not np.any(np.concatenate([g_[2] for g_ in got]) >= len(ix.masks["short"]))


def test_all_allowed_filter_equals_the_unfiltered_call(big, mse, orc):
    ix = big
    for with_url in (False, True):
        for disable_pq, beam, L in ((False, 4, 100), (True, 8, 300)):
            args = (ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.starts, ix.qh, ix.luts, SCALES, disable_pq, beam)
            a = mse.disk_search_batch(*args, search_list=L, visited_cap=4096, as_arrays=True)
            b = mse.disk_search_batch(*args, search_list=L, visited_cap=4096, as_arrays=True, filter=ix.filters["all"])
            assert sorted(a) == sorted(b)
            for key in ("buf_len", "n_visited", "cmps", "pq_cmps"):
                assert np.array_equal(a[key], b[key]), key
            for q in range(ix.nq):
                assert np.array_equal(a["buf_ids"][q, :a["buf_len"][q]], b["buf_ids"][q, :b["buf_len"][q]])
                assert np.array_equal(a["buf_scores"][q, :a["buf_len"][q]], b["buf_scores"][q, :b["buf_len"][q]])
                assert np.array_equal(a["visited_ids"][q, :a["n_visited"][q]], b["visited_ids"][q, :b["n_visited"][q]])
                assert np.array_equal(a["visited_scores"][q, :a["n_visited"][q]], b["visited_scores"][q, :b["n_visited"][q]])
            qa = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.qh, K, ix.starts, ix.luts, SCALES, disable_pq, beam, L)
            qb = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.qh, K, ix.starts, ix.luts, SCALES, disable_pq, beam, L,
                                     filter=ix.filters["all"], regime="graph")
            assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
            assert all(np.array_equal(qa[2][c], qb[2][c]) for c in ("n_visited", "cmps", "pq_cmps"))


@pytest.mark.parametrize("beam,disable_pq,L,nq", [(4, True, 16, 40), (4, False, 16, 40), (3, True, 40, 1100), (4, True, 12, 1100), (4, True, 300, 1100)])
def test_filtered_search_among_many_equal_scores(gpu, mse, orc, beam, disable_pq, L, nq):
    """The tie-heavy set of test_beam_search_among_many_equal_scores_matches_oracle (a third of the rows are exact copies), filtered:
    the four-wave kernels (small batches, every ADC-scored search, L or pre-buffer above 256) and the one-wave exact kernel (more
    than 1024 exactly scored queries, L and pre-buffer <= 256) both test the filter's bit."""
    d = 1152
    rng = np.random.default_rng(77)
    n, deg = 2400, 16
    x = clustered_rows(orc, n, d, n_centres=12)
    src, dst = rng.integers(0, n, size=n // 3), rng.choice(n, size=n // 3, replace=False)
    x[dst] = x[src]
    base = orc.f16_bits(x)
    cents, T = train_pq(orc, x[:1500], 18)
    opq, gpq = orc.PQ(cents, T, 18, d), mse.ProductQuantizer(cents, T, 18, d)
    codes = opq.quantize_batch(orc.f16_to_f32(base))
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    desc[dst] = desc[src]
    adj, degs = knn_graph(x, deg, rng)
    adj[7, 5] = adj[7, 2]
    has_url = (rng.random(n) > 0.2).astype(np.uint8)
    allowed = rng.random(n) < 0.4
    flt = mse.RowFilter(allowed)
    searcher = mse.Searcher(mse.VectorList.from_f16s(base, d))
    gcodes = mse.Codes(codes, desc)
    dgraph = mse.DeviceGraph(mse.IndexGraph(adj, degs), has_url)
    qs = clustered_rows(orc, nq, d, n_centres=12, seed=300)
    qs[::5] = x[rng.integers(0, n, size=len(qs[::5]))]
    qh = orc.f16_bits(qs)
    luts = np.zeros((nq, 64 * 256), np.float32)
    if not disable_pq:
        luts = np.stack([opq.preprocess_query(q) for q in qs])
    starts = rng.integers(0, n, size=nq).astype(np.uint32)
    got = mse.disk_search_batch(searcher, gpq, gcodes, dgraph, starts, qh, luts, SCALES, disable_pq, beam, search_list=L, visited_cap=n, filter=flt)
    url = (allowed & has_url.astype(bool)).astype(np.uint8)
    tied = kept = 0
    for i in (range(nq) if nq <= 64 else range(0, nq, 9)):
        obuf, ovids, ovsc, ocm, opc = orc.disk_greedy_search(base, adj, degs, codes, desc, int(starts[i]), qh[i], luts[i], SCALES, disable_pq, beam, L, url)
        bi, bs, vi, vs, cm, pc = got[i]
        assert (cm, pc) == (ocm, opc), i
        assert np.array_equal(bi, obuf.ids) and np.array_equal(bs, obuf.scores), i
        assert np.array_equal(vi, ovids) and np.array_equal(vs, ovsc), i
        assert np.all(url[vi] == 1)
        tied += int(len(np.unique(bs)) < len(bs))
        kept += len(vi)
    assert tied > 0 and kept > 0


@pytest.mark.parametrize("dedup", [0.0, 0.95])
def test_request_path_explicit_graph_f16_f32_entry_table_and_dedup(big, mse, orc, dedup):
    """mse_disk_query_topk_filtered / _f32 in the GRAPH regime: the sorted cut of the oracle's filtered visited list, with the handler's
    de-duplication off and at 0.95 (orc.dedup_keep in visit order first); start nodes given, and by the entry table with every entry
    node disallowed (the entry step is not filtered)."""
    ix = big
    rng = np.random.default_rng(5)
    g = ix.graphs[True]
    entry_ids = np.sort(rng.choice(N, 40, replace=False)).astype(np.uint32)
    mask = ix.masks["half"].copy()
    mask[entry_ids] = False
    flt = mse.RowFilter(mask)
    url = (mask & ix.has_url.astype(bool)).astype(np.uint8)
    L, beam = 64, 4

    def want(i, start, qh, lut, disable_pq, scales):
        _, ovids, ovsc, ocm, opc = ix.oracle(orc, i, L, beam, disable_pq, scales, url, start=start, qh=qh, lut=lut)
        nv = len(ovids)
        if dedup:
            keep = orc.dedup_keep(ix.base[ovids], dedup).astype(bool)
            ovids, ovsc = ovids[keep], ovsc[keep]
        return sorted_cut(ovids, ovsc, K) + (ocm, opc, nv)

    mse.set_entries(g, ix.vecs, entry_ids)
    mse.set_dedup(g, dedup)
    try:
        _, best = orc.bruteforce_topk(ix.base[entry_ids], ix.qh, 1)
        by_table = entry_ids[best[:, 0]]
        assert not mask[by_table].any()
        for disable_pq, scales in ((False, SCALES), (True, None)):
            for starts_arg, starts in ((ix.starts, ix.starts), (None, by_table)):
                ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, starts_arg, ix.luts, scales, disable_pq, beam, L,
                                                  filter=flt, regime="graph")
                for i in range(ix.nq):
                    wi, ws, ocm, opc, nv = want(i, starts[i], ix.qh[i], ix.luts[i], disable_pq, scales)
                    assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (disable_pq, i)
                    assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (ocm, opc, nv)
                    assert nv >= K
        # f32 queries: the RNE f16 copy scores, the tables are made from the f32 query (src/query_disk_index.rs:475-477)
        q32 = (ix.qs * np.float32(1.3)).astype(np.float32)
        q16 = orc.f16_bits(q32)
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, q32, K, ix.starts, None, SCALES, False, beam, L, filter=flt, regime="graph")
        for i in range(ix.nq):
            wi, ws, ocm, opc, nv = want(i, ix.starts[i], q16[i], ix.opq.preprocess_query(q32[i]), False, SCALES)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), i
            assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (ocm, opc, nv)
        # a one-query call (through the coalescer) is the row of the batch
        one = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, q32[3:4], K, ix.starts[3:4], None, SCALES, False, beam, L, filter=flt, regime="graph")
        assert np.array_equal(one[0][0], ids[3]) and np.array_equal(one[1][0], sc[3])
    finally:
        mse.set_dedup(g, 0.0)


def list_oracle(ix, orc, q16, eligible, scales, k):
    s = orc.score_all(ix.base, q16)
    rows = np.flatnonzero(eligible)
    sc = s[rows].copy()
    if scales is not None:
        with np.errstate(over="ignore"):
            sc = sc + np.array([orc.descriptor_product(scales, ix.desc, int(r)) for r in rows], np.int64)
    return sorted_cut(rows, sc, k)


@pytest.mark.parametrize("which", ["big", "small"])
def test_list_regime_is_the_exact_subset_sort(big, small, mse, orc, which):
    """LIST: the k best of {allowed AND has_url} by fast_dot + descriptor product, (score desc, id asc), absent rows absent: with and
    without scales, has_url = 0 rows inside the allowed set, ties by the lower id (copied rows), an allowed row whose score saturates
    (an infinite component) next to excluded ones, nq of 1, 8, 9 and 40, k beyond the eligible rows, f32 queries, and -- with the
    de-duplication on -- an error that leaves the outputs alone."""
    ix = big if which == "big" else small
    rng = np.random.default_rng(9)
    # an index of its own: copies (ties) and two saturating rows, one allowed and one not
    base = ix.base.copy()
    base[101], base[4000], base[4001] = base[100], base[17], base[17]
    base[6000, 0] = base[6001, 0] = 0xFC00                          # -inf: the dot product is infinite for every query, the score saturates
    vecs = mse.VectorList.from_f16s(base, ix.d)
    s = mse.Searcher(vecs)
    mask = rng.random(N) < 0.01
    mask[[100, 101, 17, 4000, 6000]] = True
    mask[[4001, 6001]] = False
    has_url = ix.has_url.copy()
    has_url[[100, 101, 17, 6000]] = 1
    has_url[4000] = 0                                                # allowed, but no url: absent
    assert (mask & (has_url == 0)).sum() > 3
    g_url, g_plain = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), has_url), ix.graphs[False]
    flt = mse.RowFilter(mask)
    local = Index.__new__(Index)
    local.base, local.desc = base, ix.desc
    q40 = orc.f16_bits(clustered_rows(orc, 40, ix.d, n_centres=48, seed=77))
    q40[0], q40[1] = base[100], base[17]                              # queries that ARE copied rows: equal scores at the top
    for g, eligible in ((g_url, mask & (has_url != 0)), (g_plain, mask)):
        for scales in (None, SCALES):
            for nq in (1, 8, 9, 40):
                ids, sc, st = mse.disk_query_topk(s, None, ix.gcodes, g, q40[:nq], K, None, None, scales, True, 4, 50, filter=flt, regime="list")
                for i in range(nq):
                    wi, ws = list_oracle(local, orc, q40[i], eligible, scales, K)
                    assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (nq, i)
                assert np.all(st["n_visited"] == eligible.sum()) and np.all(st["cmps"] == eligible.sum()) and np.all(st["pq_cmps"] == 0)
        # ties by the lower id; the row without a url is absent although its copy ranks first
        ids, sc, _ = mse.disk_query_topk(s, None, None, g, q40[:2], K, None, None, None, True, 4, 50, filter=flt, regime="list")
        at = list(ids[0]).index(100)                                  # (the row with the infinite component may rank above everything)
        assert ids[0][at + 1] == 101 and sc[0][at] == sc[0][at + 1]
        assert 17 in ids[1] and ((4000 in ids[1]) == (g is g_plain)) and 4001 not in ids[1]
        # k beyond the eligible rows: every eligible row, the saturated one among them, then padding; the excluded saturated row is absent
        big_k = int(eligible.sum()) + 7
        ids, sc, _ = mse.disk_query_topk(s, None, None, g, q40[:3], big_k, None, None, None, True, 4, 50, filter=flt, regime="list")
        for i in range(3):
            wi, ws = list_oracle(local, orc, q40[i], eligible, None, big_k)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws)
            assert 6000 in ids[i] and 6001 not in ids[i] and np.all(ids[i][-7:] == NONE) and np.all(sc[i][-7:] == LOWEST)
            assert sorted(ids[i][:-7]) == list(np.flatnonzero(eligible))
    # f32 queries: their RNE f16 copies score
    q32 = (clustered_rows(orc, 9, ix.d, n_centres=48, seed=78) * np.float32(1.7)).astype(np.float32)
    ids, sc, _ = mse.disk_query_topk(s, ix.gpq, ix.gcodes, g_url, q32, K, None, None, SCALES, False, 4, 50, filter=flt, regime="list")
    for i in range(9):
        wi, ws = list_oracle(local, orc, orc.f16_bits(q32[i]), mask & (has_url != 0), SCALES, K)
        assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), i
    # the de-duplication on: LIST is an error and writes nothing
    from mse import ffi
    import ctypes as C
    mse.set_dedup(g_url, 0.95)
    try:
        oi, os_ = np.full((2, K), 123, np.uint32), np.full((2, K), 456, np.int64)
        nv = np.full(2, 789, np.uint32)
        q = np.ascontiguousarray(q40[:2])
        rc = ffi.lib().mse_disk_query_topk_filtered(s._h, None, None, g_url._h, flt._h, 2, None, q.ctypes.data_as(C.POINTER(C.c_uint16)), None, None, 2, 1,
                                                    4, 50, K, oi.ctypes.data_as(C.POINTER(C.c_uint32)), os_.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    nv.ctypes.data_as(C.POINTER(C.c_uint32)), None, None)
        assert rc != 0 and "de-duplicate" in ffi.last_error()
        assert np.all(oi == 123) and np.all(os_ == 456) and np.all(nv == 789)
    finally:
        mse.set_dedup(g_url, 0.0)


def test_auto_is_the_explicit_call_at_the_plans_answer(big, mse, orc):
    """n = 20 000, L = 200: 3 907 allowed rows -> L' = 1024, GRAPH; 3 906 -> L' = 1025, LIST.  AUTO returns what the explicit call at
    mse_filtered_plan's answer returns; with the de-duplication on the sparse side runs GRAPH at 1024; no allowed row: all padding."""
    ix = big
    rng = np.random.default_rng(3)
    rows = rng.choice(N, 3907, replace=False)
    g = ix.graphs[True]
    args = (ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, SCALES, False, 4, 200)
    for count, want in ((3907, ("graph", 1024)), (3906, ("list", 200))):
        flt = mse.RowFilter(rows[:count], n_rows=N)
        assert flt.count == count and mse.filtered_plan(N, flt.count, 200) == want
        auto = mse.disk_query_topk(*args, filter=flt)
        explicit = mse.disk_query_topk(*args[:-1], want[1], filter=flt, regime=want[0])
        assert np.array_equal(auto[0], explicit[0]) and np.array_equal(auto[1], explicit[1])
        assert all(np.array_equal(auto[2][c], explicit[2][c]) for c in ("n_visited", "cmps", "pq_cmps"))
        assert np.any(auto[0] != NONE)
        if want[0] == "list":
            assert np.all(auto[2]["pq_cmps"] == 0) and np.all(auto[2]["cmps"] == (ix.has_url[rows[:count]] != 0).sum())
        else:
            assert np.all(auto[2]["pq_cmps"] > 0)
            url = np.zeros(N, np.uint8)
            url[rows[:count]] = ix.has_url[rows[:count]]
            _, ovids, ovsc, _, _ = ix.oracle(orc, 0, 1024, 4, False, SCALES, url)
            wi, ws = sorted_cut(ovids, ovsc, K)
            assert np.array_equal(auto[0][0], wi) and np.array_equal(auto[1][0], ws)
    flt = mse.RowFilter(rows[:3906], n_rows=N)
    mse.set_dedup(g, 0.95)
    try:
        assert mse.filtered_plan(N, 3906, 200, True) == ("graph", 1024)
        auto = mse.disk_query_topk(*args, filter=flt)
        explicit = mse.disk_query_topk(*args[:-1], 1024, filter=flt, regime="graph")
        assert np.array_equal(auto[0], explicit[0]) and np.array_equal(auto[1], explicit[1]) and np.all(auto[2]["pq_cmps"] > 0)
        empty = mse.disk_query_topk(*args, filter=ix.filters["none"])
        assert np.all(empty[0] == NONE) and np.all(empty[1] == LOWEST) and np.all(empty[2]["cmps"] == 0)
    finally:
        mse.set_dedup(g, 0.0)


def test_filtered_one_query_calls_and_tickets_share_submissions(big, mse, orc):
    """64 threads x one-query calls over two filter objects, both regimes, and unfiltered calls mixed: every answer equals the call
    made alone, and the coalescer shows shared submissions; tickets (QueryTickets(filter=...)) the same."""
    ix = big
    g = ix.graphs[True]
    rng = np.random.default_rng(11)
    mse.set_entries(g, ix.vecs, np.sort(rng.choice(N, 40, replace=False)).astype(np.uint32))
    T, L, beam = 64, 48, 4
    qs = clustered_rows(orc, T, ix.d, n_centres=48, seed=500).astype(np.float32)
    kinds = [dict(filter=ix.filters["half"], regime="graph"), dict(filter=ix.filters["tenth"], regime="graph"),
             dict(filter=ix.filters["pct"], regime="list"), dict(filter=ix.filters["half"], regime="auto"), dict()]
    lone = mse.Searcher(ix.vecs)
    want = [mse.disk_query_topk(lone, None, ix.gcodes, g, qs[i:i + 1], K, None, None, SCALES, True, beam, L, **kinds[i % len(kinds)]) for i in range(T)]
    assert any(np.any(w[0] != NONE) for w in want[2::5])
    got, errs = [None] * T, []
    gate = threading.Barrier(T)

    def worker(i):
        try:
            gate.wait()
            for _ in range(3):
                got[i] = mse.disk_query_topk(ix.searcher, None, ix.gcodes, g, qs[i:i + 1], K, None, None, SCALES, True, beam, L, **kinds[i % len(kinds)])
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    before = mse.coalescer_stats(g)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(T):
        assert np.array_equal(got[i][0], want[i][0]) and np.array_equal(got[i][1], want[i][1]), i
        assert all(np.array_equal(got[i][2][c], want[i][2][c]) for c in ("n_visited", "cmps", "pq_cmps")), i
    after = mse.coalescer_stats(g)
    assert after["requests"] - before["requests"] == 3 * T
    assert after["max_pass_queries"] > 1 and after["passes"] - before["passes"] < 3 * T       # requests shared submissions
    # tickets: one thread keeps all of them in flight
    tickets = [mse.QueryTickets(ix.searcher, None, ix.gcodes, g, K, True, beam, L, **kd) for kd in kinds]
    before = mse.coalescer_stats(g)
    for i in range(T):
        tickets[i % len(kinds)].submit(qs[i], SCALES, key=i)
    done = {}
    while len(done) < T:
        for key, ids, sc in tickets[0].collect(timeout_us=2_000_000):
            done[key] = (ids, sc)
    for i in range(T):
        assert np.array_equal(done[i][0], want[i][0]) and np.array_equal(done[i][1], want[i][1]), i
    after = mse.coalescer_stats(g)
    assert after["requests"] - before["requests"] == T and after["passes"] - before["passes"] < T


def test_filtered_argument_errors_write_nothing(big, mse, orc):
    """null filter, a filter longer than the graph, an unknown regime: non-zero, a message, outputs untouched -- in every entry point."""
    import ctypes as C
    from mse import ffi
    ix = big
    L = ffi.lib()
    g = ix.graphs[False]
    too_long = mse.RowFilter(np.ones(N + 1, bool))
    ok = ix.filters["half"]
    u32, i64, u16, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    q16 = np.ascontiguousarray(ix.qh[:2])
    q32 = np.ascontiguousarray(ix.qs[:2], np.float32)
    st = np.ascontiguousarray(ix.starts[:2])

    def fresh():
        return np.full((2, K), 123, np.uint32), np.full((2, K), 456, np.int64), np.full(2, 789, np.uint32)

    def untouched(oi, os_, nv):
        return np.all(oi == 123) and np.all(os_ == 456) and np.all(nv == 789)

    for flt, regime, word in ((None, 1, "null filter"), (too_long._h, 1, "longer"), (ok._h, 7, "regime"), (None, 0, "null filter"), (too_long._h, 2, "longer")):
        oi, os_, nv = fresh()
        outs = (oi.ctypes.data_as(u32), os_.ctypes.data_as(i64), nv.ctypes.data_as(u32), None, None)
        assert L.mse_disk_query_topk_filtered(ix.searcher._h, None, None, g._h, flt, regime, st.ctypes.data_as(u32), q16.ctypes.data_as(u16), None, None,
                                              2, 1, 4, 50, K, *outs) != 0
        assert word in ffi.last_error() and untouched(oi, os_, nv), (word, ffi.last_error())
        assert L.mse_disk_query_topk_filtered_f32(ix.searcher._h, None, None, g._h, flt, regime, st.ctypes.data_as(u32), q32.ctypes.data_as(f32), None,
                                                  2, 1, 4, 50, K, *outs) != 0
        assert word in ffi.last_error() and untouched(oi, os_, nv)
        t = C.c_void_p()
        assert L.mse_disk_query_submit_filtered_f32(ix.searcher._h, None, None, g._h, flt, regime, q32.ctypes.data_as(f32), None, 2, 1, 4, 50, K, *outs,
                                                    None, None, C.byref(t)) != 0
        assert word in ffi.last_error() and untouched(oi, os_, nv) and not t.value
    for flt, word in ((None, "null filter"), (too_long._h, "longer")):
        bi, bs, bl = np.full((2, 50), 123, np.uint32), np.full((2, 50), 456, np.int64), np.full(2, 789, np.uint32)
        cnt = np.full((3, 2), 789, np.uint32)
        assert L.mse_disk_search_batch_filtered(ix.searcher._h, None, None, g._h, flt, st.ctypes.data_as(u32), q16.ctypes.data_as(u16), None, None, 2, 1, 4,
                                                50, bi.ctypes.data_as(u32), bs.ctypes.data_as(i64), bl.ctypes.data_as(u32), None, None, 0,
                                                cnt[0].ctypes.data_as(u32), cnt[1].ctypes.data_as(u32), cnt[2].ctypes.data_as(u32)) != 0
        assert word in ffi.last_error() and np.all(bi == 123) and np.all(bs == 456) and np.all(bl == 789) and np.all(cnt == 789)
    with pytest.raises(mse.MseError, match="longer"):
        mse.disk_query_topk(ix.searcher, None, None, g, ix.qh[:2], K, ix.starts[:2], None, None, True, 4, 50, filter=too_long)
    with pytest.raises(mse.MseError):                                    # a filter of the right length still needs a search_list in range
        mse.disk_query_topk(ix.searcher, None, None, g, ix.qh[:2], K, ix.starts[:2], None, None, True, 4, 2000, filter=ok)
