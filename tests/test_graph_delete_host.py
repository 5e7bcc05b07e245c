"""Delete rows and repair the graph (include/mse.h), the part that needs no device: the rule restated in Python -- the yardstick of
tests/test_gpu_graph_delete.py -- and its own invariants on an oracle-built graph; the wrappers' argument checks; the three new entry
points declared, exported, bound, and failing loudly when there is nothing to run on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import SEED_CENTRES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 1152


def restate_delete(orc, rows, adj, deg, dead, cfg):
    """The rule of include/mse.h, list by list.  `dead` is the boolean delete set D; N(x) = adj[x, :deg[x]] as passed in.
    Returns (new adj, new deg, stats as mse_graph_delete_rows counts them except stats[0])."""
    dead = np.asarray(dead, bool)
    new_adj, new_deg = adj.copy(), deg.copy()
    rewritten, longest, over = 0, 0, 0
    for p in range(len(deg)):
        lst = adj[p, :deg[p]]
        if dead[p] or not dead[lst].any():
            continue                                          # 1. only live nodes that list a member of D are touched
        cand, seen = [], {p}
        for v in lst:                                         # 2. the walk, in list order
            for c in (adj[v, :deg[v]] if dead[v] else (v,)):
                c = int(c)
                if not dead[c] and c not in seen:             #    members of D, p itself and later occurrences are dropped
                    seen.add(c)
                    cand.append(c)
        ids = np.array(cand, np.uint32)
        new = np.empty(0, np.uint32)
        if ids.size:                                          # 3. fast_dot(row p, row c), then robust_prune; empty C: empty list
            new = orc.robust_prune(rows, ids, orc.score_rows(rows, ids, rows[p]), p, cfg)
        new_adj[p, :new.size] = new
        new_deg[p] = new.size
        rewritten += 1
        longest = max(longest, ids.size)
        over += ids.size > cfg.maxc
    new_deg[dead] = 0                                         # 4. every member of D ends with an empty list
    return new_adj, new_deg, {"lists_rewritten": rewritten, "max_candidates": longest, "lists_over_maxc": over}


def same_graph(adj_a, deg_a, adj_b, deg_b):
    """edge for edge: equal lengths and equal entries inside them (what lies past a list's length is not part of the graph)"""
    if not np.array_equal(deg_a, deg_b):
        return False
    live = np.arange(adj_a.shape[1])[None, :] < np.asarray(deg_a)[:, None]
    return bool(np.array_equal(adj_a[live], adj_b[live]))


def property_set(orc, n=3000, nq=200):
    """The issue's CPU-checked input: n x 1152 clustered rows (60 centres, noise 2 / sqrt(d)), held-out queries of the same kind.
    Seeds: centres SEED_CENTRES, rows 41, queries 42."""
    centres = orc.f16_to_f32(orc.gen_rows_f16(SEED_CENTRES, 0, 60))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)

    def draw(m, seed):
        rng = np.random.default_rng(seed)
        x = centres[rng.integers(0, 60, m)] + rng.standard_normal((m, D)).astype(np.float32) * np.float32(2.0 / np.sqrt(D))
        return orc.f16_bits(x / np.linalg.norm(x, axis=1, keepdims=True))
    return draw(n, 41), draw(nq, 42)


def oracle_graph(orc, rows, r=32, l=64, maxc=250, passes=2, seed=43, batch=64):
    """random fill, then `passes` build passes in a seeded order (generate_index_shard.rs:85-133), on the CPU oracle"""
    n = len(rows)
    cfg = orc.BuildConfig.make(r=r, l=l, maxc=maxc)
    adj, deg = orc.random_fill_graph(seed, n, r)
    med = orc.medioid(rows)
    rng = np.random.default_rng(seed)
    for _ in range(passes):
        orc.build_graph(rows, adj, deg, rng.permutation(n).astype(np.uint32), med, cfg, batch)
    return adj, deg, med, cfg


@pytest.fixture(scope="module")
def built(orc):
    rows, queries = property_set(orc)
    adj, deg, med, cfg = oracle_graph(orc, rows)
    return rows, queries, adj, deg, med, cfg


@pytest.mark.parametrize("frac", [0.01, 0.5])
def test_restatement_invariants(orc, built, frac):
    rows, _, adj, deg, _, cfg = built
    n = len(rows)
    dead = np.random.default_rng(int(frac * 1000)).random(n) < frac
    a1, d1, st = restate_delete(orc, rows, adj, deg, dead, cfg)
    live = ~dead
    affected = np.array([live[p] and dead[adj[p, :deg[p]]].any() for p in range(n)])
    # no live list names a deleted row; a rewritten list names neither its own node nor an id twice; deleted lists are empty
    for p in np.flatnonzero(live):
        lst = a1[p, :d1[p]]
        assert not dead[lst].any() and d1[p] <= cfg.r, p
        if affected[p]:
            assert p not in lst and len(set(lst.tolist())) == len(lst), p
    assert (d1[dead] == 0).all()
    # unaffected lists are untouched
    assert st["lists_rewritten"] == int(affected.sum()) > 0
    same = ~affected & live
    assert np.array_equal(d1[same], deg[same]) and np.array_equal(a1[same], adj[same])
    # a second call with the same D changes nothing
    a2, d2, st2 = restate_delete(orc, rows, a1, d1, dead, cfg)
    assert st2["lists_rewritten"] == 0 and same_graph(a1, d1, a2, d2)
    assert st["max_candidates"] <= cfg.r + cfg.r * cfg.r


def test_restatement_first_occurrence_and_empty_list(orc):
    """A hand-made graph: the walk order, the first occurrence, and a node left with nothing."""
    rows, _ = property_set(orc, 8, 1)
    adj = np.zeros((8, 3), np.uint32)
    deg = np.zeros(8, np.uint32)
    for p, lst in {0: [1, 2, 3], 1: [4, 2, 0], 2: [5], 3: [1, 6], 6: [7], 7: [6]}.items():
        adj[p, :len(lst)] = lst
        deg[p] = len(lst)
    dead = np.zeros(8, bool)
    dead[[1, 7]] = True
    cfg = orc.BuildConfig.make(r=3, l=8, maxc=8, saturate_graph=True)     # saturate: every candidate that fits is kept
    a, d, st = restate_delete(orc, rows, adj, deg, dead, cfg)
    assert sorted(a[0, :d[0]].tolist()) == [2, 3, 4]                       # walk of node 0: 4, 2, (0), 2, 3 -> candidates 4, 2, 3
    assert d[3] == 3 and set(a[3, :3].tolist()) <= {4, 2, 0, 6}           # walk of node 3: 4, 2, 0, 6 -> four candidates, three kept
    assert d[6] == 0 and d[1] == 0 and d[7] == 0                          # node 6 listed only node 7, whose list holds only node 6
    assert np.array_equal(a[2, :d[2]], [5]) and st["lists_rewritten"] == 3


def fake_graph(mse, cls):
    g = object.__new__(cls)
    g._h = None
    return g


@pytest.mark.parametrize("cls", ["DeviceGraph", "BuildGraph"])
def test_wrapper_argument_checks(mse, cls):
    g = fake_graph(mse, getattr(mse, cls))
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    with pytest.raises(TypeError, match="IndexBuildConfig"):
        g.delete_rows(object(), [1, 2], {"r": 32})
    for bad in (-1, 1.5, True, "8"):
        with pytest.raises(ValueError, match="batch"):
            g.delete_rows(object(), [1, 2], cfg, batch=bad)
    with pytest.raises(mse.MseError, match="searcher"):
        g.delete_rows(None, [1, 2], cfg)

    class S:
        _h = 1
    with pytest.raises(mse.MseError, match="closed"):                      # a closed graph is refused before anything is made
        g.delete_rows(S(), [1, 2], cfg)
    with pytest.raises(mse.MseError, match="closed"):
        g.deleted()
    with pytest.raises(TypeError):
        g.restore_rows(["a"])
    with pytest.raises(TypeError):
        g.restore_rows([0.5])
    with pytest.raises(ValueError):
        g.restore_rows([-1])
    with pytest.raises(mse.MseError, match="closed"):
        g.restore_rows([3])
    assert mse.DELETE_STATS == ("deleted", "lists_rewritten", "max_candidates", "lists_over_maxc")


NEW_SYMBOLS = ["mse_graph_delete_rows", "mse_graph_deleted", "mse_graph_restore_rows"]


def test_new_entry_points_are_declared_exported_and_bound():
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES and ffi.SIGNATURES[name][0] is C.c_int, name
        assert getattr(ffi.lib(), name) is not None, name
    assert len(ffi.SIGNATURES["mse_graph_delete_rows"][1]) == 6


def test_new_entry_points_fail_loudly_without_their_objects(mse):
    """No handle, no work: every entry point reports through mse_last_error and writes nothing; without a device not even a graph
    can be made, so there is nothing a delete could silently fall back to."""
    from mse import ffi
    L = ffi.lib()
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    assert L.mse_graph_delete_rows(None, None, None, C.byref(cfg), 0, stats) != 0
    assert "graph_delete_rows" in ffi.last_error() and list(stats) == [7, 7, 7, 7]
    cnt = C.c_size_t(9)
    assert L.mse_graph_deleted(None, None, C.byref(cnt)) != 0 and cnt.value == 9
    assert "graph_deleted" in ffi.last_error()
    assert L.mse_graph_restore_rows(None, None, 0) != 0
    assert "graph_restore_rows" in ffi.last_error()
    if L.mse_device_count() <= 0:
        with pytest.raises(mse.MseError):
            mse.BuildGraph(64, 8)
        with pytest.raises(mse.MseError):
            mse.DeviceGraph(mse.IndexGraph(np.zeros((64, 8), np.uint32), np.zeros(64, np.uint32)))
