"""Delete rows and repair the graph on the device (mse_graph_delete_rows) against the Python restatement of the rule in
tests/test_graph_delete_host.py: edge for edge (adj, deg, deleted map), then every search entry point on the graph deleted from ON THE
DEVICE against a fresh upload of the restatement's arrays and against the CPU oracle, slot reuse, the recall property, errors and a
delete racing the coalescer."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_gpu_filtered_graph import Index, SCALES, sorted_cut, clustered_rows
from test_graph_delete_host import restate_delete, same_graph, property_set, oracle_graph

pytestmark = pytest.mark.gpu
D, N, K = 1152, 20000, 10
NONE = 0xFFFFFFFF
KW = dict(r=32, l=64, maxc=250)


def cfgs(orc, mse, **kw):
    return orc.BuildConfig.make(**kw), mse.IndexBuildConfig(**kw)


class World:
    def __init__(self, mse, orc):
        self.base = orc.f16_bits(clustered_rows(orc, N, D, n_centres=N // 60, noise=0.5, seed=5))
        self.vecs = mse.VectorList.from_f16s(self.base, D)
        self.s = mse.Searcher(self.vecs)
        g = mse.BuildGraph(N, 32)
        g.random_fill(9)
        self.med = mse.medioid(self.vecs)
        g.build(self.s, np.random.default_rng(9).permutation(N).astype(np.uint32), self.med, mse.IndexBuildConfig(**KW), 1024)
        h = g.to_host()
        g.close()
        self.adj, self.deg = h.adj, h.deg


@pytest.fixture(scope="module")
def world(gpu, mse, orc):
    return World(mse, orc)


def delete_on_device(mse, searcher, adj, deg, dead, mcfg, batch=0, cls=None):
    n, r = adj.shape
    g = mse.BuildGraph(n, r, mse.IndexGraph(adj, deg)) if cls is None else cls(mse.IndexGraph(adj, deg))
    st = g.delete_rows(searcher, dead, mcfg, batch)
    h = g.to_host()
    return g, h.adj, h.deg, st


def check_against_restatement(mse, orc, searcher, base, adj, deg, dead, ocfg, mcfg, batches=(0,), cls=None):
    wa, wd, wst = restate_delete(orc, base, adj, deg, dead, ocfg)
    first = None
    for batch in batches:
        g, ga, gd, st = delete_on_device(mse, searcher, adj, deg, dead, mcfg, batch, cls)
        print(f"batch {batch}: {st} (restatement {wst})")
        assert same_graph(ga, gd, wa, wd), f"batch {batch}: the device graph differs from the restatement"
        assert np.array_equal(g.deleted(), dead)
        assert st["deleted"] == int(dead.sum())
        assert {k: st[k] for k in wst} == wst
        if first is None:
            first = (ga, gd)
        else:                                                   # identical, also past the ends of the lists that were rewritten
            assert np.array_equal(ga, first[0]) and np.array_equal(gd, first[1]), f"batch {batch} gives another graph"
        g.close()
    return wa, wd, wst


@pytest.mark.parametrize("frac", [0.01, 0.1, 0.5])
def test_delete_matches_restatement(world, mse, orc, frac):
    """r 32 / L 64 / maxc 250 on the device-built graph of 20 000 rows; batch 1, 7 and the default give the identical graph."""
    w = world
    dead = np.random.default_rng(int(frac * 100)).random(N) < frac
    ocfg, mcfg = cfgs(orc, mse, **KW)
    wa, wd, wst = check_against_restatement(mse, orc, w.s, w.base, w.adj, w.deg, dead, ocfg, mcfg, batches=(0, 7, 1))
    assert wst["lists_rewritten"] > 0 and wst["max_candidates"] > 32
    live = ~dead
    assert not dead[wa[live][np.arange(32)[None, :] < wd[live][:, None]]].any()


def test_in_ram_search_after_delete(world, mse, orc):
    """mse_graph_search_batch on the graph deleted from on the device == on an upload of the restatement's arrays == the oracle.
    (This entry point is the in-RAM greedy_search of lib.rs:183-211: it takes vectors and lists only and reads neither codes,
    descriptors nor has_url, so the plain graph of `world` checks all it can see; the index with codes, descriptors and a partial
    has_url is searched through the other entry points in test_search_after_delete.)"""
    w = world
    dead = np.random.default_rng(77).random(N) < 0.1
    dead[w.med] = False
    ocfg, mcfg = cfgs(orc, mse, **KW)
    wa, wd, _ = restate_delete(orc, w.base, w.adj, w.deg, dead, ocfg)
    g, ga, gd, _ = delete_on_device(mse, w.s, w.adj, w.deg, dead, mcfg)
    twin = mse.BuildGraph(N, 32, mse.IndexGraph(wa, wd))
    q = orc.f16_bits(clustered_rows(orc, 16, D, n_centres=N // 60, noise=0.5, seed=6))
    a, b = g.search_batch(w.s, w.med, q, 48), twin.search_batch(w.s, w.med, q, 48)
    for i in range(16):
        nb, dist = orc.greedy_search(w.base, wa, wd, w.med, q[i], 48)
        assert np.array_equal(a[i][0], b[i][0]) and np.array_equal(a[i][1], b[i][1]) and a[i][2] == b[i][2]
        assert np.array_equal(a[i][0], nb.ids) and np.array_equal(a[i][1], nb.scores) and a[i][2] == dist
        assert not dead[a[i][0]].any()


@pytest.mark.parametrize("kw", [dict(r=32, l=64, maxc=32), dict(r=32, l=64, maxc=250, saturate_graph=True), dict(r=32, l=64, maxc=250, alpha=78643)])
def test_delete_config_variants(world, mse, orc, kw):
    """maxc forced to 32 (candidate lists exceed it), saturate_graph, alpha = 1.2 x 2^16"""
    w = world
    dead = np.random.default_rng(3).random(N) < 0.1
    ocfg, mcfg = cfgs(orc, mse, **kw)
    wa, wd, wst = check_against_restatement(mse, orc, w.s, w.base, w.adj, w.deg, dead, ocfg, mcfg, batches=(0, 7))
    if kw["maxc"] == 32:
        assert wst["lists_over_maxc"] > wst["lists_rewritten"] // 2        # the cut to maxc really decides
    base_a, base_d, _ = restate_delete(orc, w.base, w.adj, w.deg, dead, orc.BuildConfig.make(**KW))
    assert not same_graph(wa, wd, base_a, base_d)                          # ... and each variant gives another graph than the plain config
    if kw.get("saturate_graph"):
        assert wd[~dead].mean() > base_d[~dead].mean()


def test_delete_among_exact_duplicates(gpu, mse, orc):
    """A fifth of the rows are exact copies of other rows: equal scores make the candidate ORDER decide -- first occurrence, stable
    sort."""
    n = 6000
    rng = np.random.default_rng(12)
    x = clustered_rows(orc, n, D, n_centres=40, noise=0.5, seed=13)
    dst = rng.choice(n, n // 5, replace=False)
    src = rng.choice(np.setdiff1d(np.arange(n), dst), n // 5)
    x[dst] = x[src]
    base = orc.f16_bits(x)
    vl = mse.VectorList.from_f16s(base, D)
    s = mse.Searcher(vl)
    g = mse.BuildGraph(n, 32)
    g.random_fill(14)
    g.build(s, rng.permutation(n).astype(np.uint32), mse.medioid(vl), mse.IndexBuildConfig(**KW), 512)
    h = g.to_host()
    dead = rng.random(n) < 0.3
    ocfg, mcfg = cfgs(orc, mse, **KW)
    ties = 0
    for p in np.flatnonzero(~dead)[:300]:                       # the set really has equal scores inside one list
        sc = orc.score_rows(base, h.adj[p, :h.deg[p]], base[p])
        ties += len(sc) - len(set(sc.tolist()))
    assert ties > 0
    check_against_restatement(mse, orc, s, base, h.adj, h.deg, dead, ocfg, mcfg, batches=(0, 7, 1))


def test_delete_on_a_graph_of_degree_128(gpu, mse, orc):
    """Lists longer than 64: the union of two built graphs, as merged indexes are, uploaded with max degree 128 and repaired with
    r 64 (the walk's table lives in HBM at this width)."""
    n = 4000
    base = orc.f16_bits(clustered_rows(orc, n, D, n_centres=30, noise=0.5, seed=21))
    vl = mse.VectorList.from_f16s(base, D)
    s = mse.Searcher(vl)
    med = mse.medioid(vl)
    parts = []
    for seed in (22, 23):
        g = mse.BuildGraph(n, 64)
        g.random_fill(seed)
        g.build(s, np.random.default_rng(seed).permutation(n).astype(np.uint32), med, mse.IndexBuildConfig(r=64, l=96, maxc=300, saturate_graph=True), 512)
        parts.append(g.to_host())
        g.close()
    adj, deg = np.zeros((n, 128), np.uint32), np.zeros(n, np.uint32)
    for p in range(n):
        u = list(dict.fromkeys(parts[0].adj[p, :parts[0].deg[p]].tolist() + parts[1].adj[p, :parts[1].deg[p]].tolist()))
        adj[p, :len(u)], deg[p] = u, len(u)
    assert (deg > 64).sum() > n // 5                           # lists longer than 64 are common, not a corner
    dead = np.random.default_rng(24).random(n) < 0.2
    ocfg, mcfg = cfgs(orc, mse, r=64, l=96, maxc=300)
    _, wd, wst = check_against_restatement(mse, orc, s, base, adj, deg, dead, ocfg, mcfg, batches=(0, 7), cls=mse.DeviceGraph)
    assert wst["max_candidates"] > 64 and wd.max() <= 64


def test_delete_edge_cases(world, mse, orc):
    w = world
    ocfg, mcfg = cfgs(orc, mse, **KW)
    # a node all of whose neighbours and second neighbours are deleted: its list ends empty
    p = 4321
    dead = np.zeros(N, bool)
    first = w.adj[p, :w.deg[p]]
    dead[first] = True
    for v in first:
        dead[w.adj[v, :w.deg[v]]] = True
    dead[p] = False
    wa, wd, _ = check_against_restatement(mse, orc, w.s, w.base, w.adj, w.deg, dead, ocfg, mcfg)
    assert wd[p] == 0 and w.deg[p] > 0
    # D empty: nothing changes, zero stats
    g, ga, gd, st = delete_on_device(mse, w.s, w.adj, w.deg, np.zeros(N, bool), mcfg)
    assert np.array_equal(ga, w.adj) and np.array_equal(gd, w.deg) and set(st.values()) == {0} and not g.deleted().any()
    # the same D twice: the second call rewrites nothing and counts nothing
    dead = np.random.default_rng(8).random(N) < 0.05
    st1 = g.delete_rows(w.s, dead, mcfg)
    h1 = g.to_host()
    st2 = g.delete_rows(w.s, dead, mcfg)
    h2 = g.to_host()
    assert st1["deleted"] == int(dead.sum()) and st1["lists_rewritten"] > 0
    assert st2["deleted"] == 0 and st2["lists_rewritten"] == 0 and np.array_equal(h1.adj, h2.adj) and np.array_equal(h1.deg, h2.deg)
    # D1 then D2, against the restatement applied twice (not the same as the union at once)
    d2 = np.random.default_rng(9).random(N) < 0.05
    d2 &= ~dead
    again = d2 | (dead & (np.arange(N) % 2 == 0))               # half of D1 named again: ignored and not counted
    st3 = g.delete_rows(w.s, again, mcfg)
    a1, g1, _ = restate_delete(orc, w.base, w.adj, w.deg, dead, ocfg)
    a2, g2, _ = restate_delete(orc, w.base, a1, g1, again, ocfg)
    h3 = g.to_host()
    assert same_graph(h3.adj, h3.deg, a2, g2) and np.array_equal(g.deleted(), dead | again)
    assert st3["deleted"] == int((again & ~dead).sum())
    au, gu, _ = restate_delete(orc, w.base, w.adj, w.deg, dead | again, ocfg)
    assert not same_graph(a2, g2, au, gu)
    g.close()


# ---- search after delete ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def index(gpu, mse, orc):
    return Index(mse, orc, D, 31)


def request_calls(mse, ix, g, beam=2, L=64):
    """every request-path entry point on graph g: name -> tuple of arrays"""
    out = {}
    for name, dp in (("adc", False), ("exact", True)):
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, SCALES, dp, beam, L)
        out["topk_" + name] = (ids, sc, st["n_visited"], st["cmps"], st["pq_cmps"])
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qs, K, ix.starts, None, SCALES, dp, beam, L)
        out["topk_f32_" + name] = (ids, sc, st["n_visited"], st["cmps"], st["pq_cmps"])
        a = mse.disk_search_batch(ix.searcher, ix.gpq, ix.gcodes, g, ix.starts, ix.qh, ix.luts, SCALES, dp, beam, search_list=L, visited_cap=2048,
                                  as_arrays=True)
        nv = a["n_visited"]
        assert int(nv.max()) <= 2048
        vis = np.arange(2048)[None, :] < nv[:, None]
        buf = np.arange(L)[None, :] < a["buf_len"][:, None]
        out["batch_" + name] = (a["buf_len"], nv, a["cmps"], a["pq_cmps"], a["buf_ids"][buf], a["buf_scores"][buf], a["visited_ids"][vis],
                                a["visited_scores"][vis])
    return out


def same_answers(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert np.array_equal(x, y), name


def test_search_after_delete(index, mse, orc):
    """codes, descriptors, partial has_url: the graph deleted from on the device answers as a fresh upload of the restatement's arrays
    with has_url & ~D does, bit for bit, and as the oracle does on those arrays; no deleted id in any answer."""
    ix = index
    rng = np.random.default_rng(55)
    dead = rng.random(ix.n) < 0.1
    dead[ix.starts] = False
    ocfg, mcfg = cfgs(orc, mse, r=16, l=64, maxc=250)
    wa, wd, _ = restate_delete(orc, ix.base, ix.adj, ix.degs, dead, ocfg)
    url2 = (ix.has_url.astype(bool) & ~dead).astype(np.uint8)
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    st = g.delete_rows(ix.searcher, mse.RowFilter(dead), mcfg)
    h = g.to_host()
    assert same_graph(h.adj, h.deg, wa, wd) and st["deleted"] == int(dead.sum())
    twin = mse.DeviceGraph(mse.IndexGraph(wa, wd), url2)
    got, want = request_calls(mse, ix, g), request_calls(mse, ix, twin)
    same_answers(got, want)
    for name, dp in (("adc", False), ("exact", True)):
        ids, sc, nv, cm, pc = got["topk_" + name]
        assert not dead[ids[ids != NONE]].any()
        assert not dead[got["batch_" + name][6]].any()          # visited ids
        for i in range(ix.nq):
            _, ovids, ovsc, ocm, opc = orc.disk_greedy_search(ix.base, wa, wd, ix.codes, ix.desc, int(ix.starts[i]), ix.qh[i], ix.luts[i], SCALES,
                                                             dp, 2, 64, url2)
            wi, ws = sorted_cut(ovids, ovsc, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (name, i)
            assert (int(cm[i]), int(pc[i]), int(nv[i])) == (ocm, opc, len(ovids)), (name, i)
        assert (nv >= K).all()                                  # the searches are not degenerate
    # a filtered call, GRAPH and LIST regimes, and the runtime de-duplication still match the upload twin
    for regime in ("graph", "list"):
        a = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, SCALES, False, 2, 64, filter=ix.filters["half"],
                                regime=regime)
        b = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, twin, ix.qh, K, ix.starts, ix.luts, SCALES, False, 2, 64, filter=ix.filters["half"],
                                regime=regime)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][c], b[2][c]) for c in a[2])
        assert not dead[a[0][a[0] != NONE]].any() and (a[0] != NONE).any()
    mse.set_dedup(g, 0.95)
    mse.set_dedup(twin, 0.95)
    a = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, SCALES, False, 2, 64)
    b = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, twin, ix.qh, K, ix.starts, ix.luts, SCALES, False, 2, 64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][c], b[2][c]) for c in a[2])
    g.close()
    twin.close()


def test_slot_reuse(gpu, mse, orc):
    """Base as a wrapped device tensor: delete 500 rows, overwrite them, rows_changed, restore_rows, build over them with batch 1 ==
    orc.build_graph continued on the restatement's repaired arrays with the new rows."""
    import torch
    from mse import ffi
    n = 6000
    rows = orc.f16_bits(clustered_rows(orc, n, D, n_centres=40, noise=0.5, seed=31))
    t = torch.from_numpy(rows.view(np.int16).copy()).cuda()
    vl = mse.VectorList.wrap_device(t.data_ptr(), n, D, keepalive=t)
    s = mse.Searcher(vl)
    ocfg, mcfg = cfgs(orc, mse, **KW)
    g = mse.BuildGraph(n, 32)
    g.random_fill(32)
    med = mse.medioid(vl)
    g.build(s, np.random.default_rng(32).permutation(n).astype(np.uint32), med, mcfg, 512)
    h0 = g.to_host()
    rng = np.random.default_rng(33)
    ids = rng.choice(np.setdiff1d(np.arange(n), [med]), 500, replace=False).astype(np.uint32)
    dead = np.zeros(n, bool)
    dead[ids] = True
    st = g.delete_rows(s, ids, mcfg)
    assert st["deleted"] == 500 and g.deleted().sum() == 500
    wa, wd, _ = restate_delete(orc, rows, h0.adj, h0.deg, dead, ocfg)
    fresh = orc.f16_bits(clustered_rows(orc, 500, D, n_centres=40, noise=0.5, seed=34))
    rows2 = rows.copy()
    rows2[ids] = fresh
    t.copy_(torch.from_numpy(rows2.view(np.int16)).cuda())
    torch.cuda.synchronize()
    ffi.check(ffi.lib().mse_base_rows_changed(vl._h))
    with pytest.raises(mse.MseError, match="not deleted"):
        g.restore_rows([int(np.flatnonzero(~dead)[0])])
    g.restore_rows(ids)
    assert not g.deleted().any()
    g.build(s, ids, med, mcfg, 1)
    h = g.to_host()
    orc.build_graph(rows2, wa, wd, ids, med, ocfg, 1)
    assert same_graph(h.adj, h.deg, wa, wd)
    assert (h.deg[ids] > 0).all()


def test_repair_keeps_more_recall_than_the_lazy_delete(gpu, mse, orc):
    """On the CPU-checked input (3 000 clustered rows, oracle-built r 32 / L 64 / maxc 250 graph, half the rows deleted, search list 16):
    recall@10 over the live rows of the repaired graph is not below that of the lazy delete (walk through dead nodes, drop them from
    the answer) on the same graph.  A condition, not a tolerance."""
    rows, queries = property_set(orc)
    adj, deg, med, ocfg = oracle_graph(orc, rows)
    n = len(rows)
    dead = np.random.default_rng(44).random(n) < 0.5
    dead[med] = False
    live = np.flatnonzero(~dead)
    sc = np.stack([orc.score_all(rows, q) for q in queries])
    sc[:, dead] = -(1 << 62)                                   # (not INT64_MIN: it is its own negative)
    truth = np.argsort(-sc, axis=1, kind="stable")[:, :10]
    assert not dead[truth].any()
    s = mse.Searcher(mse.VectorList.from_f16s(rows, D))
    mcfg = mse.IndexBuildConfig(**KW)
    g = mse.BuildGraph(n, 32, mse.IndexGraph(adj, deg))

    def recall(found):
        return float(np.mean([len(set(truth[i].tolist()) & set(f.tolist())) / 10.0 for i, f in enumerate(found)]))
    lazy = recall([ids[~dead[ids]][:10] for ids, _, _ in g.search_batch(s, med, queries, 16)])
    g.delete_rows(s, dead, mcfg)
    repaired = recall([ids[:10] for ids, _, _ in g.search_batch(s, med, queries, 16)])
    print(f"recall@10 at search list 16, half of {n} rows deleted: lazy {lazy:.4f}, repaired {repaired:.4f} ({len(live)} live rows)")
    assert lazy > 0.3 and repaired >= lazy


# ---- errors and concurrency --------------------------------------------------------------------------------------------------------
def test_errors_leave_the_graph_untouched(world, mse, orc):
    from mse import ffi
    w = world
    L = ffi.lib()
    mcfg = mse.IndexBuildConfig(**KW)
    g = mse.BuildGraph(N, 32, mse.IndexGraph(w.adj, w.deg))
    stats = (C.c_uint64 * 4)()

    def untouched():
        h = g.to_host()
        return np.array_equal(h.adj, w.adj) and np.array_equal(h.deg, w.deg) and not g.deleted().any()
    short = mse.RowFilter(np.ones(N - 5, bool))
    with pytest.raises(mse.MseError, match="rows"):
        g.delete_rows(w.s, short, mcfg)
    assert untouched()
    good = mse.RowFilter(np.arange(100), N)
    assert L.mse_graph_delete_rows(w.s._h, g._h, None, C.byref(mcfg), 0, stats) != 0 and "null" in ffi.last_error()
    assert L.mse_graph_delete_rows(w.s._h, g._h, good._h, None, 0, stats) != 0 and "null" in ffi.last_error()
    assert untouched()
    for bad in (dict(r=64, l=64, maxc=250), dict(r=32, l=64, maxc=2000), dict(r=0, l=64, maxc=250)):   # r above the stride, maxc, r = 0
        with pytest.raises(mse.MseError):
            g.delete_rows(w.s, good, mse.IndexBuildConfig(**bad))
    other = mse.Searcher(mse.VectorList.from_f16s(w.base[:1000], D))
    with pytest.raises(mse.MseError, match="length"):
        g.delete_rows(other, good, mcfg)
    assert untouched()
    # a node of the entry table in D: the caller moves the entry first
    mse.set_entries(g, w.vecs, np.array([50, 7000], np.uint32))
    with pytest.raises(mse.MseError, match="entry"):
        g.delete_rows(w.s, good, mcfg)
    assert untouched()
    mse.set_entry_centroids(g, orc.f16_to_f32(w.base[[60, 7000]]), np.array([60, 7000], np.uint32))
    with pytest.raises(mse.MseError, match="entry"):
        g.delete_rows(w.s, good, mcfg)
    assert untouched()
    mse.set_entries(g, w.vecs, np.array([150, 7000], np.uint32))
    assert g.delete_rows(w.s, good, mcfg)["deleted"] == 100
    with pytest.raises(mse.MseError, match="not deleted"):
        g.restore_rows([5, 5])                                  # named twice: nothing is restored
    assert g.deleted().sum() == 100
    with pytest.raises(mse.MseError, match="outside"):
        g.restore_rows([N])
    g.close()


def test_delete_races_the_coalescer(index, mse, orc):
    """One delete_rows against 64 threads of one-query disk_query_topk calls through the coalescer: every answer equals the
    before-graph's or the after-graph's answer for that query -- no error, no mixed state."""
    ix = index
    rng = np.random.default_rng(66)
    nq = 64
    qs = orc.f16_bits(clustered_rows(orc, nq, D, n_centres=48, seed=67))
    entries = rng.choice(ix.n, 32, replace=False).astype(np.uint32)
    dead = rng.random(ix.n) < 0.3
    dead[entries] = False
    mcfg = mse.IndexBuildConfig(r=16, l=64, maxc=250)
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    mse.set_entries(g, ix.vecs, entries)

    def ask(graph, i):
        ids, sc, _ = mse.disk_query_topk(ix.searcher, None, None, graph, qs[i:i + 1], K, None, None, None, True, 2, 48)
        return ids[0].copy(), sc[0].copy()
    before = [ask(g, i) for i in range(nq)]
    flt = mse.RowFilter(dead)
    answers, errors = [[] for _ in range(nq)], []
    go, done = threading.Event(), threading.Event()

    def worker(i):
        try:
            go.wait(30)
            for _ in range(5000):
                last = done.is_set()                            # one more whole request after the delete has returned
                answers[i].append(ask(g, i))
                if last:
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(nq)]
    for t in threads:
        t.start()
    go.set()
    while min(len(a) for a in answers) < 2 and not errors and any(t.is_alive() for t in threads):
        threading.Event().wait(0.002)
    st = g.delete_rows(ix.searcher, flt, mcfg)
    done.set()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "a request thread did not come back"
    assert not errors, errors[:3]
    after = [ask(g, i) for i in range(nq)]
    assert st["deleted"] == int(dead.sum())
    n_before = n_after = changed = 0
    for i in range(nq):
        changed += not np.array_equal(before[i][0], after[i][0])
        assert not dead[after[i][0][after[i][0] != NONE]].any()
        seen_after = False
        for ids, sc in answers[i]:
            is_b = np.array_equal(ids, before[i][0]) and np.array_equal(sc, before[i][1])
            is_a = np.array_equal(ids, after[i][0]) and np.array_equal(sc, after[i][1])
            assert is_b or is_a, f"query {i}: an answer that is neither the before-graph's nor the after-graph's"
            if is_a and not is_b:
                seen_after = True
            assert not (seen_after and is_b and not is_a), f"query {i}: a before-answer after an after-answer"
            n_before += is_b
            n_after += is_a and not is_b
    print(f"{n_before} answers from the graph before the delete, {n_after} from the graph after it; {changed} of {nq} queries changed their answer")
    assert changed > nq // 2 and n_before > 0 and n_after > 0
    g.close()
