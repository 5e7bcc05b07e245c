"""Compact deleted rows away and grow capacity on the device (mse_graph_compact) against the numpy restatement of the rule in
tests/test_graph_compact_host.py: every array of the new triple, both maps and the stats; the block boundaries of the map; every
request-path entry point on the new triple against a fresh upload, the CPU oracle and the old triple through the map; growth followed
by inserts; the old handles untouched and independent; errors; and a compact racing requests and a delete."""
import ctypes as C
import threading
import types

import numpy as np
import pytest

from conftest import make_pq
from test_gpu_filtered_graph import Index, SCALES, sorted_cut, clustered_rows, knn_graph
from test_gpu_graph_delete import request_calls, same_answers, cfgs
from test_graph_delete_host import same_graph, property_set, oracle_graph
from test_graph_compact_host import restate_compact

pytestmark = pytest.mark.gpu
D, K = 1152, 10
NONE = 0xFFFFFFFF
IKW = dict(r=16, l=64, maxc=250)                                 # the graphs of stride 16 (knn_graph, the Index fixture)


def compact(mse, g, searcher, codes=None, capacity=None):
    vecs, ncodes, ng, o2n, n2o = g.compact(searcher, codes, capacity)
    return types.SimpleNamespace(vecs=vecs, searcher=mse.Searcher(vecs), gcodes=ncodes, g=ng, o2n=o2n, n2o=n2o, stats=ng.compact_stats)


def check_triple(t, c, cap):
    """every array of the new triple t == the restatement c"""
    assert len(t.vecs) == cap and np.array_equal(t.vecs.rows(0, cap), c.rows)
    if c.codes is not None:
        assert len(t.gcodes) == cap
        if c.desc is not None:
            gc, gd = t.gcodes.read_rows(0, cap, descriptors=True)
            assert np.array_equal(gd, c.desc)
        else:
            gc = t.gcodes.read_rows(0, cap)
        assert np.array_equal(gc, c.codes)
    else:
        assert t.gcodes is None
    h = t.g.to_host()
    assert h.adj.shape == c.adj.shape and np.array_equal(h.deg, c.deg)
    assert np.array_equal(h.adj, c.adj)                          # also past the ends of the lists: zeros, as a fresh graph has them
    assert np.array_equal(t.g.deleted(), c.deleted if c.deleted is not None else np.zeros(cap, bool))
    assert np.array_equal(t.o2n, c.old_to_new) and np.array_equal(t.n2o, c.new_to_old)
    assert t.stats == c.stats, (t.stats, c.stats)


# ---- 1. arrays equal the restatement -----------------------------------------------------------------------------------------------
N1 = 2999                                                        # no multiple of 32, 64 or 256


class Small:
    def __init__(self, mse, orc):
        rng = np.random.default_rng(101)
        self.x = clustered_rows(orc, N1, D, n_centres=20, seed=102)
        self.rows = orc.f16_bits(self.x)
        cents, T, dpc, _ = make_pq(orc, D, D // 64)
        self.opq, self.gpq = orc.PQ(cents, T, dpc, D), mse.ProductQuantizer(cents, T, dpc, D)
        self.codes = self.opq.quantize_batch(orc.f16_to_f32(self.rows))
        self.desc = rng.integers(0, 256, size=(N1, 4), dtype=np.uint8)
        self.adj, self.deg = knn_graph(self.x, 16, rng)
        self.has_url = (rng.random(N1) > 0.15).astype(np.uint8)
        self.entry = 1500
        self.keep = np.concatenate([[self.entry], rng.choice(np.setdiff1d(np.arange(N1), [self.entry]), 40, replace=False)])
        self.has_url[self.keep] = 1
        self.vecs = mse.VectorList.from_f16s(self.rows, D)
        self.searcher = mse.Searcher(self.vecs)
        self.gcodes = mse.Codes(self.codes, self.desc)
        self.qh = orc.f16_bits(clustered_rows(orc, 6, D, n_centres=20, seed=103))
        self.luts = np.stack([self.opq.preprocess_query(q) for q in orc.f16_to_f32(self.qh)])
        self.ocfg, self.mcfg = cfgs(orc, mse, **IKW)

    def pattern(self, name):
        ids = {"none": [], "row 0": [0], "the last row": [N1 - 1], "a bitmap word": list(range(64, 96)), "rows 31..33": [31, 32, 33],
               "every second row": list(range(1, N1, 2)), "all but 41": np.setdiff1d(np.arange(N1), self.keep).tolist()}[name]
        dead = np.zeros(N1, bool)
        dead[ids] = True
        return dead


@pytest.fixture(scope="module")
def small(gpu, mse, orc):
    return Small(mse, orc)


@pytest.mark.parametrize("name", ["none", "row 0", "the last row", "a bitmap word", "rows 31..33", "every second row", "all but 41"])
def test_arrays_equal_the_restatement(small, mse, orc, name):
    w = small
    dead = w.pattern(name)
    url = None if name == "none" else w.has_url                  # "none": a graph without a has_url array that was never deleted from
    g = mse.DeviceGraph(mse.IndexGraph(w.adj, w.deg), url)
    if dead.any():
        assert g.delete_rows(w.searcher, np.flatnonzero(dead), w.mcfg)["deleted"] == int(dead.sum())
    h = g.to_host()
    url_now = None if url is None else (url.astype(bool) & ~dead).astype(np.uint8)
    n_live = int((~dead).sum())
    starts = np.full(len(w.qh), w.entry, np.uint32)
    for cap in (n_live, n_live + 1, N1 + 1000):
        c = restate_compact(w.rows, w.codes, w.desc, h.adj, h.deg, url_now, dead, cap)
        t = compact(mse, g, w.searcher, w.gcodes, cap)
        check_triple(t, c, cap)
        assert (c.has_url is None) == (name == "none" and cap == n_live)
        # has_url, seen through the searches: the new triple answers as a fresh upload of the restated arrays, flags included
        twin_v = mse.VectorList.from_f16s(c.rows, D)
        twin = types.SimpleNamespace(searcher=mse.Searcher(twin_v), gcodes=mse.Codes(c.codes, c.desc), g=mse.DeviceGraph(mse.IndexGraph(c.adj, c.deg), c.has_url))
        st2 = c.old_to_new[starts]
        for dp in (False, True):
            a = mse.disk_query_topk(t.searcher, w.gpq, t.gcodes, t.g, w.qh, K, st2, w.luts, SCALES, dp, 2, 64)
            b = mse.disk_query_topk(twin.searcher, w.gpq, twin.gcodes, twin.g, w.qh, K, st2, w.luts, SCALES, dp, 2, 64)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
            found = a[0][a[0] != NONE]
            assert found.size and (found < n_live).all()
            if c.has_url is not None:
                assert c.has_url[found].all()                    # a row with has_url = 0 is never returned
        t.g.close()
        twin.g.close()
    # the default capacity is the live count
    vecs, codes, g2, o2n, n2o = g.compact(w.searcher)
    assert len(vecs) == n_live == len(n2o) and codes is None and g2.compact_stats["bytes_moved"] == n_live * D * 2
    g2.close()
    g.close()


def test_default_capacity_is_the_live_count_the_call_saw(small, mse, orc):
    """The wrapper reads the live count and hands it to the call, which takes the lock on its own: a writer can slip in between.  Here
    the count the wrapper reads first is made stale on purpose -- too high, as after a concurrent delete (the call succeeds with a
    spare tail nobody asked for), then too low, as after a concurrent insert (the call refuses) -- and the wrapper must come back with
    the tail-free triple of the true count both times.  Also: new_to_old has `capacity` entries however far the index grows."""
    w = small
    dead = w.pattern("every second row")
    g = mse.DeviceGraph(mse.IndexGraph(w.adj, w.deg), w.has_url)
    g.delete_rows(w.searcher, np.flatnonzero(dead), w.mcfg)
    h = g.to_host()
    n_live = int((~dead).sum())
    c = restate_compact(w.rows, w.codes, w.desc, h.adj, h.deg, (w.has_url.astype(bool) & ~dead).astype(np.uint8), dead, n_live)
    real = g._live_count
    assert real() == n_live
    for off in (7, -3):
        calls = []

        def stale():
            calls.append(1)
            return real() + off if len(calls) == 1 else real()
        g._live_count = stale
        t = compact(mse, g, w.searcher, w.gcodes)
        assert len(calls) >= 2
        check_triple(t, c, n_live)
        assert t.stats["live"] == t.stats["capacity"] == len(t.vecs) == n_live
        t.g.close()
    g._live_count = lambda: real() + 7                          # a count that never settles: an error, not a wrong index
    with pytest.raises(mse.MseError, match="live count changed"):
        g.compact(w.searcher)
    del g._live_count
    cap = (1 << 20) + 5                                         # far above 4 n
    vecs, _, g2, o2n, n2o = g.compact(w.searcher, capacity=cap)
    assert len(n2o) == cap == len(vecs) and np.array_equal(n2o[:n_live], np.flatnonzero(~dead)) and (n2o[n_live:] == NONE).all()
    assert g2.deleted().sum() == cap - n_live
    g2.close()
    vecs.close()
    g.close()


# ---- 2. block boundaries of the map ---------------------------------------------------------------------------------------------------
def test_map_block_boundaries(gpu, mse, orc):
    """70 001 rows: the filter compaction (filter.hip) works in blocks of 256 bitmap words = 8 192 rows, so this is 8 full blocks and a
    partial one (2 188 words, the last with 17 rows): the block counts, their exclusive prefix (one block per thread of the one-workgroup
    scan, nine threads busy) and the in-block scan are each crossed more than once; so are the 32-row words, the 16-row workgroups of
    the row gather and the 32-node workgroups of the remap.  (The scan's several-blocks-per-thread path starts above 2 097 152 rows --
    4.8 GB of rows -- and is left to the probe.)"""
    n, r = 70001, 8
    vl = mse.VectorList.generate(0x5EED0011, 0, n)
    s = mse.Searcher(vl)
    g = mse.BuildGraph(n, r)
    g.random_fill(5, r)
    dead = np.random.default_rng(6).random(n) < 0.5
    dead[0] = False
    assert g.delete_rows(s, dead, mse.IndexBuildConfig(r=r, l=32, maxc=64))["deleted"] == int(dead.sum())
    h = g.to_host()
    live = np.flatnonzero(~dead)
    assert s.compact_timing(1) == 0.0
    vecs, _, g2, o2n, n2o = g.compact(s)
    ms = s.compact_timing(0)
    assert ms > 0.0 and s.compact_timing(0) == 0.0              # the gather kernel's own time; switched off, it reads 0 again
    print(f"row gather of {live.size} x {D * 2} bytes: {ms:.3f} ms = {2 * live.size * D * 2 / ms / 1e6:.0f} GB/s read + written (one run, small)")
    assert np.array_equal(n2o, live.astype(np.uint32))
    want = np.where(dead, NONE, np.cumsum(~dead) - 1).astype(np.uint32)
    assert np.array_equal(o2n, want)
    h2 = g2.to_host()
    assert len(vecs) == live.size and h2.adj.shape == (live.size, r) and not g2.deleted().any()
    assert np.array_equal(h2.deg, h.deg[live]) and g2.compact_stats["edges_rewritten"] == int(h.deg[live].sum())
    rng = np.random.default_rng(7)
    for new in np.concatenate([[0, live.size - 1], rng.choice(live.size, 198, replace=False)]):
        old = int(live[new])
        assert np.array_equal(vecs.rows(int(new), 1), vl.rows(old, 1)), new
        lst = h.adj[old, :h.deg[old]]
        assert not dead[lst].any()
        assert np.array_equal(h2.adj[new, :h2.deg[new]], want[lst]) and not h2.adj[new, h2.deg[new]:].any(), new
    g2.close()
    g.close()


# ---- 3. searches ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def index(gpu, mse, orc):
    return Index(mse, orc, D, 31)


class Old:
    """A private copy of the Index fixture's device objects with `frac` of the rows deleted on the device (never a start node)."""

    def __init__(self, mse, orc, ix, seed, frac=1.0 / 3.0):
        rng = np.random.default_rng(seed)
        self.ix = ix
        self.vecs = mse.VectorList.from_f16s(ix.base, D)
        self.searcher = mse.Searcher(self.vecs)
        self.gcodes = mse.Codes(ix.codes, ix.desc)
        self.g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
        self.dead = rng.random(ix.n) < frac
        self.dead[ix.starts] = False
        self.ocfg, self.mcfg = cfgs(orc, mse, **IKW)
        assert self.g.delete_rows(self.searcher, self.dead, self.mcfg)["deleted"] == int(self.dead.sum())
        self.h = self.g.to_host()
        self.url = (ix.has_url.astype(bool) & ~self.dead).astype(np.uint8)

    def restate(self, cap):
        ix = self.ix
        return restate_compact(ix.base, ix.codes, ix.desc, self.h.adj, self.h.deg, self.url, self.dead, cap)

    def view(self, t, starts):
        ix = self.ix
        return types.SimpleNamespace(searcher=t.searcher, gpq=ix.gpq, gcodes=t.gcodes, qh=ix.qh, qs=ix.qs, starts=starts, luts=ix.luts)


def map_ids(o2n, ids):
    out = np.asarray(ids, np.uint32).copy()
    out[out != NONE] = o2n[out[out != NONE]]
    return out


def test_searches_on_the_new_triple(index, mse, orc):
    ix = index
    old = Old(mse, orc, ix, 111)
    n_live = int((~old.dead).sum())
    c = old.restate(n_live)
    t = compact(mse, old.g, old.searcher, old.gcodes)
    check_triple(t, c, n_live)
    st2 = c.old_to_new[ix.starts]
    got = request_calls(mse, old.view(t, st2), t.g)
    # a fresh upload of the restated arrays, bit for bit
    tv = mse.VectorList.from_f16s(c.rows, D)
    twin = types.SimpleNamespace(searcher=mse.Searcher(tv), gcodes=mse.Codes(c.codes, c.desc), g=mse.DeviceGraph(mse.IndexGraph(c.adj, c.deg), c.has_url))
    same_answers(got, request_calls(mse, old.view(twin, st2), twin.g))
    # the oracle on them
    for name, dp in (("adc", False), ("exact", True)):
        ids, sc, nv, cm, pc = got["topk_" + name]
        for i in range(ix.nq):
            _, ovids, ovsc, ocm, opc = orc.disk_greedy_search(c.rows, c.adj, c.deg, c.codes, c.desc, int(st2[i]), ix.qh[i], ix.luts[i], SCALES, dp, 2, 64,
                                                             c.has_url)
            wi, ws = sorted_cut(ovids, ovsc, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (name, i)
            assert (int(cm[i]), int(pc[i]), int(nv[i])) == (ocm, opc, len(ovids)), (name, i)
        assert (nv >= K).all()
    # the old triple's answers with ids sent through old_to_new: scores and counters bit-equal (tests/test_graph_compact_host.py)
    was = request_calls(mse, old.view(old, ix.starts), old.g)
    assert sorted(was) == sorted(got)
    for name in was:
        a, b = was[name], got[name]
        if name.startswith("topk"):
            assert np.array_equal(map_ids(t.o2n, a[0]), b[0]), name
            rest = range(1, 5)
        else:                                                    # (buf_len, n_visited, cmps, pq_cmps, buf ids, buf scores, visited ids, visited scores)
            assert np.array_equal(map_ids(t.o2n, a[4]), b[4]) and np.array_equal(map_ids(t.o2n, a[6]), b[6]), name
            rest = (0, 1, 2, 3, 5, 7)
        for j in rest:
            assert np.array_equal(a[j], b[j]), (name, j)
    # the entry table, set again through the map
    entries = np.random.default_rng(112).choice(np.flatnonzero(~old.dead), 32, replace=False).astype(np.uint32)
    mse.set_entries(old.g, old.vecs, entries)
    mse.set_entries(t.g, t.vecs, t.o2n[entries])
    a = mse.disk_query_topk(old.searcher, ix.gpq, old.gcodes, old.g, ix.qh, K, None, ix.luts, SCALES, False, 2, 64)
    b = mse.disk_query_topk(t.searcher, ix.gpq, t.gcodes, t.g, ix.qh, K, None, ix.luts, SCALES, False, 2, 64)
    assert np.array_equal(map_ids(t.o2n, a[0]), b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    # brute force over the new base == the oracle over the live rows
    ws, wi = orc.bruteforce_topk(ix.base[~old.dead], ix.qh, K)
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA):
        gs, gi = t.searcher.bruteforce_topk(ix.qh[:8], K, mode)
        assert np.array_equal(gi, wi[:8]) and np.array_equal(gs, ws[:8]), mode
    for x in (t.g, twin.g, old.g):
        x.close()


# ---- 4. growth, then insert ----------------------------------------------------------------------------------------------------------
def test_growth_then_insert(gpu, mse, orc):
    """test_spare_slot_capacity's shape, but the capacity comes from compact and not from the first upload: 2 000 live rows with no spare,
    compacted to 3 000, two inserts of 500 into the spare tail == the oracle's continued build, edge for edge."""
    rows, _ = property_set(orc)
    n, live = len(rows), 2000
    adj0, deg0, med, ocfg = oracle_graph(orc, rows[:live])
    mcfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    vl0 = mse.VectorList.from_f16s(rows[:live], D)
    s0 = mse.Searcher(vl0)
    g0 = mse.BuildGraph(live, 32, mse.IndexGraph(adj0, deg0))
    vl, _, g, o2n, n2o = g0.compact(s0, capacity=n)
    assert np.array_equal(o2n, np.arange(live)) and np.array_equal(n2o[:live], np.arange(live)) and (n2o[live:] == NONE).all()
    assert isinstance(g, mse.BuildGraph) and (g.n, g.r) == (n, 32) and g.deleted().sum() == n - live
    g0.close()
    s = mse.Searcher(vl)
    spare = np.arange(live, n, dtype=np.uint32)
    wa, wd = np.zeros((n, 32), np.uint32), np.zeros(n, np.uint32)
    wa[:live], wd[:live] = adj0, deg0
    now = rows.copy()
    now[live:] = 0
    for part in (spare[:500], spare[500:]):
        assert g.insert_rows(s, part, rows[part], mcfg, med, batch=64) == {"inserted": 500, "batches": 8}
        now[part] = rows[part]
        orc.build_graph(now, wa, wd, part, med, ocfg, 64)
        h = g.to_host()
        assert same_graph(h.adj, h.deg, wa, wd)
    assert not g.deleted().any() and np.array_equal(vl.rows(0, n), rows) and (wd[live:] > 0).all()
    twin_s = mse.Searcher(mse.VectorList.from_f16s(rows, D))
    twin = mse.BuildGraph(n, 32, mse.IndexGraph(wa, wd))
    a, b = g.search_batch(s, med, rows[live:live + 64], 16), twin.search_batch(twin_s, med, rows[live:live + 64], 16)
    for (ai, asc, ad), (bi, bsc, bd) in zip(a, b):
        assert np.array_equal(ai, bi) and np.array_equal(asc, bsc) and ad == bd
    assert sum(int(len(ids) > 0 and ids[0] == live + i) for i, (ids, _, _) in enumerate(a)) > 0
    g.close()
    twin.close()


# ---- 5. the old handles are untouched and independent -----------------------------------------------------------------------------------
def test_old_handles_are_untouched_and_independent(index, mse, orc):
    ix = index
    old = Old(mse, orc, ix, 121, frac=0.1)
    rows0 = old.vecs.rows(0, ix.n)
    codes0, desc0 = old.gcodes.read_rows(0, ix.n, descriptors=True)
    assert np.array_equal(rows0, ix.base) and np.array_equal(codes0, ix.codes) and np.array_equal(desc0, ix.desc)
    was = request_calls(mse, old.view(old, ix.starts), old.g)
    cap = ix.n + 100
    t = compact(mse, old.g, old.searcher, old.gcodes, cap)
    c = old.restate(cap)

    def old_untouched(answers=was, dead=old.dead, h=old.h):
        h1 = old.g.to_host()
        assert np.array_equal(h1.adj, h.adj) and np.array_equal(h1.deg, h.deg) and np.array_equal(old.g.deleted(), dead)
        assert np.array_equal(old.vecs.rows(0, ix.n), rows0)
        c1, d1 = old.gcodes.read_rows(0, ix.n, descriptors=True)
        assert np.array_equal(c1, codes0) and np.array_equal(d1, desc0)
        same_answers(request_calls(mse, old.view(old, ix.starts), old.g), answers)
    old_untouched()
    st2 = t.o2n[ix.starts]
    new_was = request_calls(mse, old.view(t, st2), t.g)
    # a delete from the new graph leaves the old one as it was
    rng = np.random.default_rng(122)
    seen = np.setdiff1d(np.unique(new_was["batch_exact"][6]), st2)[:20]      # visited by the queries: the delete changes their answers
    drop = np.union1d(seen, rng.choice(np.setdiff1d(np.arange(c.n_live), st2), 280, replace=False))
    assert t.g.delete_rows(t.searcher, drop, old.mcfg)["deleted"] == drop.size
    old_untouched()
    new_after = request_calls(mse, old.view(t, st2), t.g)
    # an insert into the old graph leaves the new one as it is
    slots = np.flatnonzero(old.dead)[:200].astype(np.uint32)
    fresh = orc.f16_bits(clustered_rows(orc, 200, D, n_centres=48, seed=123))
    assert old.g.insert_rows(old.searcher, slots, fresh, old.mcfg, int(ix.starts[0]), quantizer=ix.gpq, codes=old.gcodes,
                             descriptors=desc0[slots], batch=64)["inserted"] == 200
    same_answers(request_calls(mse, old.view(t, st2), t.g), new_after)
    assert np.array_equal(t.vecs.rows(0, cap), c.rows)
    assert any(not np.array_equal(x, y) for name in new_was for x, y in zip(new_was[name], new_after[name]))   # (the delete was visible)
    # the old handles freed first: the new ones go on working
    old.g.close()
    old.gcodes.close()
    old.searcher.close()
    old.vecs.close()
    same_answers(request_calls(mse, old.view(t, st2), t.g), new_after)
    t.g.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_return_nothing_and_leave_the_old_index_as_it_was(index, mse, orc):
    from mse import ffi
    ix = index
    L = ffi.lib()
    old = Old(mse, orc, ix, 131, frac=0.1)
    n_live = int((~old.dead).sum())
    was = request_calls(mse, old.view(old, ix.starts), old.g)

    def refused(match, s=old.searcher, g=old.g, codes=old.gcodes, cap=n_live, outs="bcg"):
        bo, co, go = C.c_void_p(5), C.c_void_p(6), C.c_void_p(7)
        stats = (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = L.mse_graph_compact(s._h if s is not None else None, g._h if g is not None else None, codes._h if codes is not None else None, cap, C.byref(bo) if "b" in outs else None,
                                 C.byref(co) if "c" in outs else None, C.byref(go) if "g" in outs else None, None, None, stats)
        assert rc != 0 and match in ffi.last_error(), (match, ffi.last_error())
        assert (bo.value, co.value, go.value, list(stats)) == (5, 6, 7, [7, 7, 7, 7])   # the out pointers are untouched
        h = old.g.to_host()
        assert np.array_equal(h.adj, old.h.adj) and np.array_equal(h.deg, old.h.deg) and np.array_equal(old.g.deleted(), old.dead)
    refused("below the", cap=n_live - 1)
    refused("capacity must be", cap=0)
    refused("capacity must be", cap=0xFFFFFFFF)
    short = mse.Codes(ix.codes[:1000], ix.desc[:1000])
    refused("codes speak for 1000 rows", codes=short)
    other = mse.Searcher(mse.VectorList.from_f16s(ix.base[:1000], D))
    refused("differ in length", s=other)
    refused("null argument", s=None)
    refused("null argument", g=None)
    refused("null argument", outs="cg")
    refused("null argument", outs="bc")
    refused("null argument", outs="bg")                          # codes given, but no place for the new ones
    refused("null argument", codes=None)                         # a place for new codes, but none given
    refused("bytes of device memory are free", cap=200_000_000)  # 460 GB of rows: the first allocation fails, nothing is held
    with pytest.raises(mse.MseError, match="below the"):
        old.g.compact(old.searcher, old.gcodes, 5)
    same_answers(request_calls(mse, old.view(old, ix.starts), old.g), was)
    # ... and the same call without a mistake goes through
    t = compact(mse, old.g, old.searcher, old.gcodes)
    t.g.close(), t.gcodes.close(), t.searcher.close(), t.vecs.close()
    # a live list that names a deleted row: mse_graph_random_fill tops lists up with uniformly drawn ids and does not look at the deleted
    # map (it takes no part in the graph's lock either: include/mse.h), so after a delete it names deleted rows in live lists
    bg = mse.BuildGraph(ix.n, 16, mse.IndexGraph(old.h.adj, old.h.deg))
    assert bg.delete_rows(old.searcher, old.dead, old.mcfg)["lists_rewritten"] == 0   # the lists are repaired already: only the marks are set
    bg.random_fill(9)
    hb = bg.to_host()
    live_lists = hb.adj[~old.dead]
    inside = np.arange(16)[None, :] < hb.deg[~old.dead][:, None]
    assert old.dead[live_lists[inside]].any()                    # the public calls have made a live list that names a deleted row
    with pytest.raises(mse.MseError, match="names a deleted row"):
        bg.compact(old.searcher)
    h2 = bg.to_host()
    assert np.array_equal(h2.adj, hb.adj) and np.array_equal(h2.deg, hb.deg)
    bg.close()
    old.g.close()


# ---- 7. concurrency --------------------------------------------------------------------------------------------------------------------
def test_compact_beside_requests_and_a_delete(index, mse, orc):
    """compact runs while 16 threads send requests to the old graph and one thread runs a delete_rows: every request equals the
    before-delete or the after-delete answer, and the compacted index is the restatement of exactly one of the two states.  One run."""
    ix = index
    old = Old(mse, orc, ix, 141, frac=0.1)
    rng = np.random.default_rng(142)
    nq = 16
    qs = orc.f16_bits(clustered_rows(orc, nq, D, n_centres=48, seed=143))
    entries = rng.choice(np.flatnonzero(~old.dead), 32, replace=False).astype(np.uint32)
    second = (rng.random(ix.n) < 0.2) & ~old.dead
    second[entries] = False
    mse.set_entries(old.g, old.vecs, entries)
    del_searcher = mse.Searcher(old.vecs)                        # the delete's own stream and scratch

    def ask(i):
        ids, sc, _ = mse.disk_query_topk(old.searcher, None, None, old.g, qs[i:i + 1], K, None, None, None, True, 2, 48)
        return ids[0].copy(), sc[0].copy()
    before = [ask(i) for i in range(nq)]
    answers, errors, result = [[] for _ in range(nq)], [], {}
    go, done = threading.Event(), threading.Event()

    def worker(i):
        try:
            go.wait(30)
            for _ in range(5000):
                last = done.is_set()                             # one more whole request after both calls have returned
                answers[i].append(ask(i))
                if last:
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def deleter():
        try:
            go.wait(30)
            result["delete"] = old.g.delete_rows(del_searcher, second, old.mcfg)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(nq)]
    dt = threading.Thread(target=deleter, daemon=True)
    for th in threads + [dt]:
        th.start()
    go.set()
    t = compact(mse, old.g, old.searcher, old.gcodes)
    dt.join(120)
    done.set()
    for th in threads:
        th.join(120)
    assert not dt.is_alive() and not any(th.is_alive() for th in threads), "a thread did not come back"
    assert not errors, errors[:3]
    assert result["delete"]["deleted"] == int(second.sum())
    after = [ask(i) for i in range(nq)]
    for i in range(nq):
        for ids, sc in answers[i]:
            is_b = np.array_equal(ids, before[i][0]) and np.array_equal(sc, before[i][1])
            is_a = np.array_equal(ids, after[i][0]) and np.array_equal(sc, after[i][1])
            assert is_b or is_a, f"query {i}: an answer that is neither the before-delete nor the after-delete answer"
    # the compacted index: the restatement of the state before the delete, or of the state after it -- nothing in between
    h_after = old.g.to_host()
    dead_after = old.dead | second
    n_got = t.stats["live"]                                     # the live count the call saw under the lock: it names the state
    assert len(t.vecs) == n_got == t.stats["capacity"] and not t.g.deleted().any()   # the default capacity: never a spare tail
    state = {int((~old.dead).sum()): "before", int((~dead_after).sum()): "after"}[n_got]
    if state == "before":
        c = old.restate(n_got)
    else:
        c = restate_compact(ix.base, ix.codes, ix.desc, h_after.adj, h_after.deg, (ix.has_url.astype(bool) & ~dead_after).astype(np.uint8), dead_after, n_got)
    check_triple(t, c, n_got)
    print(f"the compacted index is the state {state} the delete; {sum(len(a) for a in answers)} requests answered meanwhile")
    t.g.close()
    old.g.close()
