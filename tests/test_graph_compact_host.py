"""Compact deleted rows away and grow capacity (mse_graph_compact, include/mse.h), the part that needs no device: the rule restated in
numpy -- the yardstick of tests/test_gpu_graph_compact.py --, the claim that makes compaction safe checked on the CPU oracle (a search
on the repaired arrays and on the compacted arrays returns the same scores, the same ids after mapping and the same counters), the
wrappers' argument checks, and the entry points failing loudly when there is nothing to run on."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import make_pq
from test_graph_delete_host import restate_delete, property_set, oracle_graph, fake_graph

D = 1152
NONE = 0xFFFFFFFF
SCALES = np.array([0.5, 0, -0.25, 1.0], np.float32) / np.float32(512)


def restate_compact(rows, codes, desc, adj, deg, has_url, deleted, capacity):
    """The rule of include/mse.h in numpy.  rows [n, d]; codes / desc [n, .] or None; adj [n, S], deg [n]; has_url [n] or None;
    deleted: boolean [n] (None: nothing deleted).  Returns a namespace of the new arrays (codes / desc / has_url / deleted None where
    the new triple has none), both maps and the stats."""
    n, S = adj.shape
    dead = np.zeros(n, bool) if deleted is None else np.asarray(deleted, bool)
    live = np.flatnonzero(~dead).astype(np.uint32)                # ascending old ids: the renumbering is monotone
    n_live = live.size
    assert 0 < capacity <= 0xFFFFFFFE and capacity >= n_live
    old_to_new = np.full(n, NONE, np.uint32)
    old_to_new[live] = np.arange(n_live, dtype=np.uint32)
    new_to_old = np.full(capacity, NONE, np.uint32)
    new_to_old[:n_live] = live

    def moved(a):                                                 # row new = row old; the spare tail is zero
        if a is None:
            return None
        out = np.zeros((capacity,) + a.shape[1:], a.dtype)
        out[:n_live] = a[live]
        return out
    new_deg = moved(deg)
    inside = np.arange(S)[None, :] < new_deg[:n_live, None]      # entries below the length, of the live lists
    old_lists = adj[live]
    assert (old_lists[inside] < n).all() and not dead[old_lists[inside]].any(), "a live list names a deleted row or a row outside the graph"
    new_adj = np.zeros((capacity, S), np.uint32)                  # entries at or past the length: 0, as mse_graph_new leaves them
    new_adj[:n_live][inside] = old_to_new[old_lists[inside]]
    tail = capacity > n_live
    url = has_url if has_url is not None or not tail else np.ones(n, np.uint8)
    new_deleted = None
    if tail:
        new_deleted = np.zeros(capacity, bool)
        new_deleted[n_live:] = True
    row_bytes = rows.shape[1] * 2 + (codes.shape[1] if codes is not None else 0) + (desc.shape[1] if codes is not None and desc is not None else 0)
    return types.SimpleNamespace(rows=moved(rows), codes=moved(codes), desc=moved(desc) if codes is not None else None, adj=new_adj, deg=new_deg,
                                 has_url=moved(None if url is None else np.asarray(url, np.uint8)), deleted=new_deleted, old_to_new=old_to_new,
                                 new_to_old=new_to_old, n_live=n_live,
                                 stats={"live": n_live, "capacity": capacity, "edges_rewritten": int(new_deg.sum()), "bytes_moved": n_live * row_bytes})


def test_restatement_on_a_hand_made_graph():
    rows = np.arange(6 * 8, dtype=np.uint16).reshape(6, 8)
    adj = np.array([[1, 3, 9], [0, 5, 5], [4, 4, 4], [5, 0, 1], [2, 2, 2], [3, 7, 7]], np.uint32)      # entries past the length: anything
    deg = np.array([2, 2, 0, 3, 1, 1], np.uint32)
    dead = np.array([0, 0, 1, 0, 1, 0], bool)
    codes, desc = np.arange(12, dtype=np.uint8).reshape(6, 2), np.arange(6, dtype=np.uint8).reshape(6, 1)
    c = restate_compact(rows, codes, desc, adj, deg, None, dead, 6)
    assert c.old_to_new.tolist() == [0, 1, NONE, 2, NONE, 3] and c.new_to_old.tolist() == [0, 1, 3, 5, NONE, NONE]
    assert c.adj.tolist() == [[1, 2, 0], [0, 3, 0], [3, 0, 1], [2, 0, 0], [0, 0, 0], [0, 0, 0]] and c.deg.tolist() == [2, 2, 3, 1, 0, 0]
    assert c.has_url.tolist() == [1, 1, 1, 1, 0, 0] and c.deleted.tolist() == [0, 0, 0, 0, 1, 1]
    assert np.array_equal(c.rows[:4], rows[[0, 1, 3, 5]]) and not c.rows[4:].any() and np.array_equal(c.codes[:4], codes[[0, 1, 3, 5]])
    assert c.desc[:, 0].tolist() == [0, 1, 3, 5, 0, 0]
    assert c.stats == {"live": 4, "capacity": 6, "edges_rewritten": 8, "bytes_moved": 4 * (16 + 2 + 1)}
    tight = restate_compact(rows, None, None, adj, deg, None, dead, 4)                                  # no spare tail: no flags, no map
    assert tight.has_url is None and tight.deleted is None and tight.codes is None and tight.stats["bytes_moved"] == 64
    with pytest.raises(AssertionError, match="names a deleted row"):
        restate_compact(rows, None, None, adj, deg, None, np.array([0, 1, 0, 0, 0, 0], bool), 6)       # row 0 lists row 1
    with pytest.raises(AssertionError):
        restate_compact(rows, None, None, adj, deg, None, dead, 3)                                      # below the live count


@pytest.fixture(scope="module")
def repaired(orc):
    """3 000 clustered rows, the oracle's graph with the delete tests' parameters, a third of the rows deleted by the restated rule;
    codes of a synthetic codec, descriptors, a has_url array with holes."""
    rows, queries = property_set(orc)
    adj, deg, med, cfg = oracle_graph(orc, rows)
    n = len(rows)
    rng = np.random.default_rng(61)
    dead = rng.random(n) < 1.0 / 3.0
    starts = rng.choice(np.flatnonzero(~dead), 12, replace=False).astype(np.uint32)
    dead[med] = False
    a1, d1, _ = restate_delete(orc, rows, adj, deg, dead, cfg)
    pq = orc.PQ(*make_pq(orc, D, D // 64))                        # 64 chunks of 18 dimensions
    codes = pq.quantize_batch(orc.f16_to_f32(rows))
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    url = ((rng.random(n) > 0.1) & ~dead).astype(np.uint8)        # what the delete leaves: has_url AND NOT D
    url[starts[:2]] = 1
    luts = np.stack([pq.preprocess_query(q) for q in orc.f16_to_f32(queries[:12])])
    return types.SimpleNamespace(rows=rows, queries=queries[:12], adj=a1, deg=d1, dead=dead, starts=starts, codes=codes, desc=desc, url=url,
                                 luts=luts, n=n)


@pytest.mark.parametrize("capacity", ["live", "grown"])
@pytest.mark.parametrize("disable_pq", [False, True])
@pytest.mark.parametrize("scales", [True, False])
def test_a_search_cannot_tell_the_compacted_arrays_from_the_repaired_ones(orc, repaired, capacity, disable_pq, scales):
    """orc.disk_greedy_search, ADC and exact, with and without descriptor scales, on the repaired arrays and on the compacted arrays:
    the same scores, the same ids after mapping (search list and visited list, in their order), the same comparison counters."""
    w = repaired
    cap = int((~w.dead).sum()) if capacity == "live" else w.n + 500
    c = restate_compact(w.rows, w.codes, w.desc, w.adj, w.deg, w.url, w.dead, cap)
    assert c.n_live == int((~w.dead).sum()) < w.n and (np.diff(c.new_to_old[:c.n_live].astype(np.int64)) > 0).all()
    sc = SCALES if scales else None
    visited = 0
    for i in range(len(w.queries)):
        ob, ovi, ovs, ocm, opc = orc.disk_greedy_search(w.rows, w.adj, w.deg, w.codes, w.desc, int(w.starts[i]), w.queries[i], w.luts[i], sc,
                                                        disable_pq, 2, 64, w.url)
        nb, nvi, nvs, ncm, npc = orc.disk_greedy_search(c.rows, c.adj, c.deg, c.codes, c.desc, int(c.old_to_new[w.starts[i]]), w.queries[i],
                                                        w.luts[i], sc, disable_pq, 2, 64, c.has_url)
        assert not w.dead[ovi].any() and not w.dead[ob.ids].any()                 # after the repair no live list reaches a dead node
        assert np.array_equal(c.old_to_new[ovi], nvi) and np.array_equal(ovs, nvs), i
        assert np.array_equal(c.old_to_new[ob.ids], nb.ids) and np.array_equal(ob.scores, nb.scores), i
        assert (ocm, opc, len(ovi)) == (ncm, npc, len(nvi)), i
        assert (nvi < c.n_live).all()                                               # the spare tail is never reached
        # the request path's last step orders by (score desc, id asc): a monotone map keeps the ties where they were
        order_old = sorted(range(len(ovi)), key=lambda j: (-int(ovs[j]), int(ovi[j])))
        order_new = sorted(range(len(nvi)), key=lambda j: (-int(nvs[j]), int(nvi[j])))
        assert order_old == order_new, i
        visited += len(ovi)
    assert visited > 12 * 10                                                        # the searches are not degenerate


@pytest.mark.parametrize("cls", ["DeviceGraph", "BuildGraph"])
def test_wrapper_argument_checks(mse, cls):
    g = fake_graph(mse, getattr(mse, cls))

    class S:
        _h = 1
    with pytest.raises(mse.MseError, match="searcher"):
        g.compact(None)
    with pytest.raises(mse.MseError, match="closed"):                              # a closed graph is refused before anything is made
        g.compact(S())
    closed = object.__new__(mse.Codes)
    closed._h = None
    with pytest.raises(mse.MseError, match="codes are closed"):
        g.compact(S(), codes=closed)
    with pytest.raises(ValueError, match="row range"):
        four = type("FourCodes", (mse.Codes,), {"__len__": lambda self: 4, "__del__": lambda self: None})
        object.__new__(four).read_rows(3, 2)
    assert mse.COMPACT_STATS == ("live", "capacity", "edges_rewritten", "bytes_moved")


def test_new_entry_points_are_bound_and_fail_loudly_without_their_objects(mse):
    from mse import ffi
    L = ffi.lib()
    assert len(ffi.SIGNATURES["mse_graph_compact"][1]) == 10 and len(ffi.SIGNATURES["mse_codes_read_rows"][1]) == 5
    bo, go = C.c_void_p(5), C.c_void_p(6)
    stats = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert L.mse_graph_compact(None, None, None, 10, C.byref(bo), None, C.byref(go), None, None, stats) != 0
    assert "graph_compact" in ffi.last_error() and "null" in ffi.last_error()
    assert (bo.value, go.value, list(stats)) == (5, 6, [7, 7, 7, 7])
    ms = C.c_double(3.5)
    assert L.mse_searcher_compact_timing(None, 1, C.byref(ms)) != 0 and "searcher_compact_timing" in ffi.last_error() and ms.value == 3.5
    out = (C.c_uint8 * 4)(9, 9, 9, 9)
    assert L.mse_codes_read_rows(None, 0, 1, out, None) != 0 and "codes_read_rows" in ffi.last_error() and list(out) == [9, 9, 9, 9]
