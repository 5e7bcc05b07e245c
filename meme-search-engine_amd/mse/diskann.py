"""Host mirror of the `diskann` crate's search pieces (reference: diskann/src/lib.rs)."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr
from .vector import Codes, RowFilter, Searcher, VectorList, _bits, _p


class NeighbourBuffer:
    """lib.rs:74-155: candidate list sorted by score descending, bounded by `size`."""

    def __init__(self, size):
        self._h = check_ptr(ffi.lib().mse_nb_new(size), "mse_nb_new")

    def insert(self, idx, score):
        ffi.lib().mse_nb_insert(self._h, int(idx), int(score))

    def next_unvisited(self):
        out = C.c_uint32()
        return int(out.value) if ffi.lib().mse_nb_next_unvisited(self._h, C.byref(out)) else None

    def clear(self):
        ffi.lib().mse_nb_clear(self._h)

    def __len__(self):
        return int(ffi.lib().mse_nb_len(self._h))

    def len(self):
        return len(self)

    def cap(self):
        return int(ffi.lib().mse_nb_cap(self._h))

    @property
    def ids(self):
        n = len(self)
        return np.ctypeslib.as_array(ffi.lib().mse_nb_ids(self._h), (n,)).copy() if n else np.empty(0, np.uint32)

    @property
    def scores(self):
        n = len(self)
        return np.ctypeslib.as_array(ffi.lib().mse_nb_scores(self._h), (n,)).copy() if n else np.empty(0, np.int64)

    def close(self):
        if self._h:
            ffi.lib().mse_nb_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IndexGraph:
    """lib.rs:16-39 as a fixed-degree table: adj[n][max_deg], deg[n]."""

    def __init__(self, adj, deg):
        self.adj = np.ascontiguousarray(adj, np.uint32)
        self.deg = np.ascontiguousarray(deg, np.uint32)


def medioid(vecs):
    """lib.rs:52-68: id of the row closest to the (f16-rounded, running-mean) centroid."""
    out = C.c_uint32()
    check(ffi.lib().mse_medioid(vecs._h, C.byref(out)), "medioid")
    return int(out.value)


def select_shard(centroids, query):
    """query_disk_index.rs:254-256,447-450: index of the shard whose centroid has the largest dot with the query
    (last maximum on ties)."""
    c = np.ascontiguousarray(centroids, np.float32)
    q = np.ascontiguousarray(query, np.float32).reshape(-1)
    if c.ndim != 2 or c.shape[1] != q.size:
        raise MseError("centroids must be [n_shards, d]")
    out = C.c_size_t()
    check(ffi.lib().mse_select_shard(_p(c, C.c_float), c.shape[0], c.shape[1], _p(q, C.c_float), C.byref(out)), "select_shard")
    return int(out.value)


DUPLICATES_THRESHOLD = 0.95   # query_disk_index.rs:99


def dedup_visited(searcher: Searcher, visited_ids, threshold=DUPLICATES_THRESHOLD):
    """query_disk_index.rs:482-527: boolean keep mask over the visited list (visit order)."""
    ids = np.ascontiguousarray(visited_ids, np.uint32)
    keep = np.zeros(ids.size, np.uint8)
    check(ffi.lib().mse_dedup_visited(searcher._h, _p(ids, C.c_uint32), ids.size, float(threshold), _p(keep, C.c_uint8)),
          "dedup_visited")
    return keep.astype(bool)


class DiskSearchResult:
    """What query_disk_index::greedy_search leaves behind: the Scratch's neighbour buffer and visited list
    (ids + exact scores, fetch order) and the returned (cmps, pq_cmps)."""

    def __init__(self, buffer, visited_ids, visited_scores, cmps, pq_cmps):
        self.neighbour_buffer = buffer
        self.visited_ids = visited_ids
        self.visited_scores = visited_scores
        self.cmps = cmps
        self.pq_cmps = pq_cmps


def disk_greedy_search(searcher: Searcher, quantizer, codes, graph: IndexGraph, start, query, query_preprocessed,
                       descriptor_scales=None, disable_pq=False, beamwidth=1, search_list=1000, has_url=None):
    """query_disk_index.rs:144-212 with the index HBM-resident.  `searcher` wraps the record vectors, `codes` the PQ
    codes + descriptor bytes, `graph` the adjacency, `query_preprocessed` a QueryLUT, `search_list` = capacity of
    the NeighbourBuffer (config.search_list / 1000 in evaluate, :288)."""
    q = _bits(query).reshape(-1)
    table = getattr(query_preprocessed, "table", query_preprocessed)
    table = np.ascontiguousarray(table, np.float32)
    sc = None if descriptor_scales is None else np.ascontiguousarray(descriptor_scales, np.float32)
    hu = None if has_url is None else np.ascontiguousarray(has_url, np.uint8)
    n = len(codes)
    buf = NeighbourBuffer(search_list)
    vids = np.empty(n, np.uint32)
    vsc = np.empty(n, np.int64)
    nv, cm, pc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(ffi.lib().mse_disk_greedy_search(
        searcher._h, quantizer._h, codes._h, _p(graph.adj, C.c_uint32), _p(graph.deg, C.c_uint32), graph.adj.shape[1],
        _p(hu, C.c_uint8) if hu is not None else None, int(start), _p(q, C.c_uint16), _p(table, C.c_float),
        _p(sc, C.c_float) if sc is not None else None, int(bool(disable_pq)), int(beamwidth), buf._h,
        _p(vids, C.c_uint32), _p(vsc, C.c_int64), n, C.byref(nv), C.byref(cm), C.byref(pc)), "disk_greedy_search")
    k = int(nv.value)
    return DiskSearchResult(buf, vids[:k].copy(), vsc[:k].copy(), int(cm.value), int(pc.value))


DELETE_STATS = ("deleted", "lists_rewritten", "max_candidates", "lists_over_maxc")   # stats[0..4) of mse_graph_delete_rows
INSERT_STATS = ("inserted", "batches")                                               # stats[0..2) of mse_graph_insert_rows
COMPACT_STATS = ("live", "capacity", "edges_rewritten", "bytes_moved")               # stats_out[0..4) of mse_graph_compact


class _DeviceRows:
    """The rows of a VectorList in the shape insert_rows takes device rows in (data_ptr() and what it checks beside it)."""

    is_cuda = True

    def __init__(self, vecs):
        self._vecs = vecs

    def data_ptr(self):
        return int(self._vecs.device_ptr or 0)

    def numel(self):
        return len(self._vecs) * self._vecs.d_emb

    def element_size(self):
        return 2

    def is_contiguous(self):
        return True


class _RowDeletes:
    """delete_rows / deleted / restore_rows / insert_rows of the two classes that wrap an mse_graph (include/mse.h "delete rows and
    repair the graph", "insert rows into freed slots")."""

    def _graph_handle(self):
        h = getattr(self, "_h", None)
        if not h:
            raise MseError("the graph is closed")
        return h

    def _n_rows(self):
        return int(ffi.lib().mse_graph_len(self._graph_handle()))

    def to_host(self) -> IndexGraph:
        """The adjacency as it is in HBM now: adj [n, max_degree], deg [n]."""
        h = self._graph_handle()
        n, r = self._n_rows(), int(ffi.lib().mse_graph_max_degree(h))
        adj, deg = np.empty((n, r), np.uint32), np.empty(n, np.uint32)
        check(ffi.lib().mse_graph_to_host(h, _p(adj, C.c_uint32), _p(deg, C.c_uint32)), "graph_to_host")
        return IndexGraph(adj, deg)

    def live_filter(self, and_has_url=False) -> RowFilter:
        """The graph's live rows as a RowFilter (mse_graph_live_filter): a row is allowed when it is not in the deleted map and -- with
        and_has_url, on a graph that has has_url flags -- its flag is set.  Built on the device; a snapshot: deletes, restores and
        inserts made later need a new filter.  With it ProductQuantizer.scan_topk*_filtered and Searcher.bruteforce_topk(allow=...)
        serve a mutated index without compact()."""
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_graph_live_filter(self._graph_handle(), int(bool(and_has_url))),
                                               "graph_live_filter"))

    def near_duplicates(self, searcher: Searcher, threshold, **kw):
        """Searcher.near_duplicates over the graph's rows within live_filter() (has_url is not consulted): deleted slots hold stale rows and
        do not pair.  within=... narrows it further.  Like every brute-force scan over a graph's base it takes no part in the graph's
        lock: the caller keeps delete_rows, insert_rows and restores on this graph out while it runs."""
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("near_duplicates needs the searcher over the graph's rows")
        live = self.live_filter(False)
        within = kw.pop("within", None)
        both = None
        try:
            if within is not None:
                if not isinstance(within, RowFilter):
                    raise TypeError("within must be a RowFilter")
                both = live & within
            return searcher.near_duplicates(threshold, within=both if both is not None else live, **kw)
        finally:
            live.close()
            if both is not None:
                both.close()

    def near_duplicates_of(self, searcher: Searcher, incoming, threshold, **kw):
        """Searcher.near_duplicates_of over the graph's rows within live_filter() (has_url is not consulted): deleted slots hold stale rows
        and do not pair.  within=... narrows it further.  Like every brute-force scan over a graph's base it takes no part in the graph's
        lock: the caller keeps delete_rows, insert_rows and restores on this graph out while it runs."""
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("near_duplicates_of needs the searcher over the graph's rows")
        live = self.live_filter(False)
        within = kw.pop("within", None)
        both = None
        try:
            if within is not None:
                if not isinstance(within, RowFilter):
                    raise TypeError("within must be a RowFilter")
                both = live & within
            return searcher.near_duplicates_of(incoming, threshold, within=both if both is not None else live, **kw)
        finally:
            live.close()
            if both is not None:
                both.close()

    def insert_unique_rows(self, searcher: Searcher, slots, rows, threshold, config, start, quantizer=None, codes=None, descriptors=None,
                           has_url=None, batch=0):
        """insert_rows of the rows that are new: a row of `rows` is inserted unless it scores >= threshold against a live row of the index or
        against an earlier row of `rows` that is itself inserted (the keep-first rule, continued from the index into the batch).
        Steps: near_duplicates_of within the live rows; near_duplicates of the batch itself; RowPairs.admit; insert_rows of the kept rows,
        with their descriptors and flags, into the first kept.count slots.  rows: a VectorList, or a numpy array of f16 values / uint16
        bits (one row per slot); the kept rows are gathered on the device and do not return to the host.  The other arguments are
        insert_rows'.
        Returns {"kept": boolean mask over rows, "rep_base", "rep_incoming": the Admission's arrays, "unused_slots": the slots left over,
        "inserted", "batches": what insert_rows returns}.
        Like every brute-force scan over a graph's base the two joins take no part in the graph's lock, and nothing holds it between the
        join and the insert: the caller keeps delete_rows, insert_rows and restores on this graph out while it runs."""
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("insert_unique_rows needs the searcher over the graph's rows")
        sl = np.asarray(slots).reshape(-1)
        owned = not isinstance(rows, VectorList)
        q = VectorList.from_f16s(rows, searcher.vecs.d_emb) if owned else rows
        qs = cross = among = adm = picked = None
        try:
            m = len(q)
            if sl.size != m:
                raise ValueError(f"one slot per row: {sl.size} slots for {m} rows")
            cross = self.near_duplicates_of(searcher, q, threshold)
            qs = Searcher(q)
            among = qs.near_duplicates(threshold)
            adm = cross.admit(among)
            kept = adm.kept.to_mask()
            k = int(adm.kept.count)
            out = {"kept": kept, "rep_base": adm.rep_base, "rep_incoming": adm.rep_incoming, "unused_slots": sl[k:].copy(),
                   "inserted": 0, "batches": 0}
            if k:
                picked = q.select(adm.kept)
                de = None if descriptors is None else np.ascontiguousarray(descriptors, np.uint8).reshape(m, -1)[kept]
                hu = None if has_url is None else np.ascontiguousarray(has_url, np.uint8).reshape(-1)[kept]
                out.update(self.insert_rows(searcher, sl[:k], _DeviceRows(picked), config, start, quantizer, codes, de, hu, batch))
            return out
        finally:
            for h in (picked, adm, among, cross, qs):
                if h is not None:
                    h.close()
            if owned:
                q.close()

    def delete_rows(self, searcher: Searcher, ids_or_filter, config, batch=0):
        """Remove rows from the live graph and repair the lists that pointed at them, on the device (mse_graph_delete_rows).
        ids_or_filter: a RowFilter over the graph's rows whose SET bits name the rows to remove, a boolean mask with one entry per row, or
        an integer array of row ids.  config: an IndexBuildConfig (r, maxc, alpha, saturate_graph are used).  batch: affected nodes per
        group of launches (0 = default; the result does not depend on it).  Returns {"deleted", "lists_rewritten", "max_candidates",
        "lists_over_maxc"}."""
        if not isinstance(config, ffi.BuildConfig):
            raise TypeError("config must be an IndexBuildConfig")
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 0:
            raise ValueError("batch must be a non-negative integer (0 = default)")
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("delete_rows needs the searcher over the graph's rows")
        h = self._graph_handle()
        owned = False
        if isinstance(ids_or_filter, RowFilter):
            flt = ids_or_filter
        else:
            a = np.asarray(ids_or_filter)
            if a.dtype != np.bool_ and not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
                raise TypeError("ids_or_filter must be a RowFilter, a boolean mask or an integer id array")
            n = self._n_rows()
            if a.dtype == np.bool_:
                if a.size != n:
                    raise ValueError(f"a boolean mask has one entry per row: {a.size} entries for a graph of {n} rows")
                flt = RowFilter(a)
            else:
                a = a.reshape(-1).astype(np.int64)
                if a.size and (a.min() < 0 or a.max() >= n):
                    raise ValueError(f"row ids must be in 0 .. {n - 1}")
                flt = RowFilter(a, n)
            owned = True
        try:
            out = (C.c_uint64 * 4)()
            check(ffi.lib().mse_graph_delete_rows(searcher._h, h, flt._h, C.byref(config), int(batch), out), "graph_delete_rows")
        finally:
            if owned:
                flt.close()
        return {name: int(out[i]) for i, name in enumerate(DELETE_STATS)}

    def deleted(self):
        """Boolean array over the graph's rows: True where the row has been deleted (and not restored)."""
        h = self._graph_handle()
        out = np.zeros(self._n_rows(), np.uint8)
        cnt = C.c_size_t()
        check(ffi.lib().mse_graph_deleted(h, _p(out, C.c_uint8), C.byref(cnt)), "graph_deleted")
        return out.astype(bool)

    def restore_rows(self, ids):
        """Give freed slots back (mse_graph_restore_rows): every id must be a deleted row, named once.  The rows count as live again
        (has_url = 1) with EMPTY lists: write their new vectors, tell the base (rows_changed) and run build() over them.  insert_rows
        does all of that, codes included, in one call under the graph's lock."""
        a = np.asarray(ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("ids must be an integer array")
        a = a.reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("row ids must be in 0 .. 2**32 - 1")
        i = np.ascontiguousarray(a, np.uint32)
        check(ffi.lib().mse_graph_restore_rows(self._graph_handle(), _p(i, C.c_uint32), i.size), "graph_restore_rows")


    def insert_rows(self, searcher: Searcher, slots, rows, config, start, quantizer=None, codes=None, descriptors=None, has_url=None, batch=0):
        """Put new vectors into free slots of the live index (mse_graph_insert_rows): rows, PQ codes, descriptors and flags are written and
        the nodes linked, in one call that the request path sees wholly before or wholly after.
        slots: integer ids of deleted rows, each once (capacity: upload spare rows with empty lists and delete_rows them).  rows: one
        f16 row per slot -- a numpy array (np.float16 or uint16 bits), or anything with data_ptr() that lies on the searcher's device
        (a torch tensor of 2-byte elements, contiguous: mse_graph_insert_rows_dev).  config: an IndexBuildConfig whose r is the graph's
        stride.  start: the node the link searches start from (the medioid).  quantizer + codes: the index's ProductQuantizer and Codes,
        both or neither; descriptors [m, n_desc] uint8 exactly when the codes carry descriptors.  has_url [m] (default: all 1).
        batch: new nodes linked per group of launches (0 = default); the graph depends on it as build()'s does.
        Returns {"inserted", "batches"}."""
        if not isinstance(config, ffi.BuildConfig):
            raise TypeError("config must be an IndexBuildConfig")
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 0:
            raise ValueError("batch must be a non-negative integer (0 = default)")
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("insert_rows needs the searcher over the graph's rows")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start <= 0xFFFFFFFF:
            raise ValueError("start must be a row id")
        h = self._graph_handle()
        sl = np.asarray(slots)
        if sl.size and not np.issubdtype(sl.dtype, np.integer):
            raise TypeError("slots must be an integer array")
        sl = sl.reshape(-1)
        if sl.size and (sl.min() < 0 or sl.max() > 0xFFFFFFFF):
            raise ValueError("slots must be in 0 .. 2**32 - 1")
        sl = np.ascontiguousarray(sl, np.uint32)
        m = sl.size
        vecs = getattr(searcher, "vecs", None)   # the width comes from the searcher's rows: a short array must not reach the library
        if vecs is None or getattr(vecs, "_h", None) is None:
            raise MseError("insert_rows needs the searcher over the graph's rows")
        d = int(vecs.d_emb)
        on_device = hasattr(rows, "data_ptr")
        if on_device:
            if not getattr(rows, "is_cuda", True):
                raise TypeError("rows with data_ptr() must lie on the searcher's device")
            if hasattr(rows, "is_contiguous") and not rows.is_contiguous():
                raise ValueError("device rows must be contiguous")
            if hasattr(rows, "element_size") and rows.element_size() != 2:
                raise TypeError("device rows must be f16 (2-byte elements)")
            n_elem = int(rows.numel())
            if n_elem != m * d:
                raise ValueError(f"rows must hold one row of the index's width per slot: {n_elem} elements for {m} slots")
            rp = C.c_void_p(int(rows.data_ptr()))
        else:
            r = _bits(rows)
            if r.size != m * d:
                raise ValueError(f"rows must hold one row of the index's width per slot: {r.size} elements for {m} slots")
            r = r.reshape(m, d)
            rp = _p(r, C.c_uint16)
        dp = up = None
        if descriptors is not None:
            de = np.ascontiguousarray(descriptors, np.uint8)
            if m == 0 or de.size == 0 or de.size % m:
                raise ValueError("descriptors must be [len(slots), n_desc]")
            de = de.reshape(m, -1)
            dp = _p(de, C.c_uint8)
        if has_url is not None:
            hu = np.ascontiguousarray(has_url, np.uint8).reshape(-1)
            if hu.size != m:
                raise ValueError("has_url has one entry per slot")
            up = _p(hu, C.c_uint8)
        out = (C.c_uint64 * 2)()
        fn = ffi.lib().mse_graph_insert_rows_dev if on_device else ffi.lib().mse_graph_insert_rows
        check(fn(searcher._h, h, quantizer._h if quantizer is not None else None, codes._h if codes is not None else None, _p(sl, C.c_uint32), m,
                 rp, dp, up, int(start), C.byref(config), int(batch), out), "graph_insert_rows")
        return {name: int(out[i]) for i, name in enumerate(INSERT_STATS)}

    def _live_count(self):
        cnt = C.c_size_t()
        check(ffi.lib().mse_graph_deleted(self._graph_handle(), None, C.byref(cnt)), "graph_deleted")
        return self._n_rows() - int(cnt.value)

    def _compact_once(self, searcher, codes, capacity):
        h = self._graph_handle()
        n = self._n_rows()
        o2n = np.empty(n, np.uint32)
        # (a capacity outside 1 .. 2^32 - 2 is refused by the call before it writes anything: no array is made for it)
        n2o = np.empty(capacity, np.uint32) if 0 < capacity <= 0xFFFFFFFE else None
        bo, co, go = C.c_void_p(), C.c_void_p(), C.c_void_p()
        out = (C.c_uint64 * 4)()
        check(ffi.lib().mse_graph_compact(searcher._h, h, codes._h if codes is not None else None, capacity, C.byref(bo),
                                          C.byref(co) if codes is not None else None, C.byref(go), _p(o2n, C.c_uint32),
                                          _p(n2o, C.c_uint32) if n2o is not None else None, out), "graph_compact")
        vecs = VectorList(bo.value)
        new_codes = None
        if codes is not None:
            new_codes = Codes.__new__(Codes)
            new_codes._h = co.value
            new_codes.code_size, new_codes.n_desc = codes.code_size, codes.n_desc
        g = object.__new__(type(self))
        g._h = go.value
        if isinstance(self, BuildGraph):
            g.n, g.r = capacity, int(ffi.lib().mse_graph_max_degree(go.value))
        g.compact_stats = {name: int(out[i]) for i, name in enumerate(COMPACT_STATS)}
        return vecs, new_codes, g, o2n, n2o

    def compact(self, searcher: Searcher, codes=None, capacity=None):
        """Repack the live index into a fresh triple of `capacity` rows on the device (mse_graph_compact): the live rows renumbered densely
        in their old order, the spare tail (capacity above the live count) marked deleted, ready for insert_rows.  Out of place: this
        graph, the searcher's rows and `codes` are only read and stay valid; both indexes are resident until the old one is closed.
        searcher: over the rows this graph indexes.  codes: the index's Codes, or None.
        capacity: rows of the new triple.  None = the live count AS THE CALL FINDS IT UNDER THE GRAPH'S LOCK: the count is read first and
        handed to the call; if a delete_rows / insert_rows / restore_rows on another thread changed it in between (the call reports the
        live count it saw), that result is released and the call repeated, so the returned triple never has a spare tail:
        len(vecs) == compact_stats["live"].  MseError if the count changes eight times in a row.
        Returns (VectorList, Codes or None, graph of this class, old_to_new [n] uint32, new_to_old [capacity] uint32); 0xFFFFFFFF marks
        a deleted row / a spare slot.  The new graph's stats are in its .compact_stats ({"live", "capacity", "edges_rewritten",
        "bytes_moved"}).  The entry table, the dedup threshold and the coalescer settings are not carried over: set them on the new
        graph, node ids through old_to_new."""
        if searcher is None or getattr(searcher, "_h", None) is None:
            raise MseError("compact needs the searcher over the graph's rows")
        if codes is not None and getattr(codes, "_h", None) is None:
            raise MseError("compact: the codes are closed")
        self._graph_handle()
        if capacity is not None:
            if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
                raise ValueError("capacity must be a non-negative integer")
            return self._compact_once(searcher, codes, int(capacity))
        for _ in range(8):
            want = self._live_count()
            try:
                got = self._compact_once(searcher, codes, want)
            except MseError:
                if self._live_count() != want:      # an insert made the count outgrow the capacity meanwhile: again
                    continue
                raise
            if got[2].compact_stats["live"] == want:
                return got
            got[2].close()                          # a delete slipped in between the count and the call: a spare tail nobody asked for
            if got[1] is not None:
                got[1].close()
            got[0].close()
        raise MseError("compact: the live count changed on every attempt; pass a capacity, or keep writers out")


class DeviceGraph(_RowDeletes):
    """Adjacency (and the has-url flags of the records) resident in HBM for disk_search_batch."""

    def __init__(self, graph: IndexGraph, has_url=None):
        hu = None if has_url is None else np.ascontiguousarray(has_url, np.uint8)
        self._h = check_ptr(ffi.lib().mse_graph_from_host(_p(graph.adj, C.c_uint32), _p(graph.deg, C.c_uint32), graph.adj.shape[0],
                                                          graph.adj.shape[1], _p(hu, C.c_uint8) if hu is not None else None),
                            "mse_graph_from_host")

    def describe(self, codes: Codes, scores, cdfs, ids=None, first=0):
        """Codes.describe on the live index's codes under this graph's exclusive lock (as insert_rows): request-path calls see the rows'
        descriptor bytes wholly before or wholly after.  ids: the rows scores' entries belong to, e.g. the slots just inserted."""
        codes.describe(scores, cdfs, ids, first, _graph=self._graph_handle())

    def encode_features(self, sae, vecs_or_searcher, **kw):
        """SparseAutoencoder.encode_rows over the index's rows, e.g. ids=the slots just inserted; RowFeatures.filter(...) of the result
        goes wherever a filter over the graph's rows does (delete_rows, the filtered searches)."""
        return sae.encode_rows(vecs_or_searcher, **kw)

    def train_features(self, trainer, vecs_or_searcher, ids, batch_size):
        """SaeTrainer.train over the index's rows `ids` (live slots, in the order given)."""
        return trainer.train(vecs_or_searcher, ids, batch_size)

    def train_rater(self, trainer, vecs_or_searcher, pairs, ratings, epochs, rng, batch_size=1):
        """RaterTrainer.train over rated pairs of the index's rows (live slots)."""
        return trainer.train(vecs_or_searcher, pairs, ratings, epochs, rng, batch_size)

    def rate_pairs(self, rater, vecs_or_searcher, a, b, k):
        """The k candidate pairs (a[i], b[i]) of the index's rows that the rater's members disagree on most, as MemberScores.top_pairs
        gives them: the rows that occur are scored once, member by member, and the pairs ranked over that table."""
        a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        rows, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
        table = rater.member_scores(vecs_or_searcher, ids=rows)
        return table.top_pairs(inv[:a.size], inv[a.size:], k)

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_graph_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


REGIMES = {"auto": 0, "graph": 1, "list": 2}   # MSE_FILTERED_*
_REGIME_NAMES = {v: k for k, v in REGIMES.items()}


def _regime(regime):
    try:
        return REGIMES[regime] if isinstance(regime, str) else int(regime)
    except KeyError:
        raise ValueError(f"regime must be one of {sorted(REGIMES)}") from None


def _filter_array(filter, nq):
    """A filter per query: `filter` as the [nq] handle array of the *_filtered_each calls (None entries: unfiltered), or None when it
    is a single RowFilter.  The array holds the RowFilter objects (._keep), so they live as long as it does, whatever kind of iterable
    they came from: the caller keeps the array until the call has returned."""
    if filter is None or isinstance(filter, RowFilter):
        return None
    fs = list(filter)
    if len(fs) != nq:
        raise MseError(f"a filter per query: {len(fs)} filters for {nq} queries")
    for f in fs:
        if f is not None and not isinstance(f, RowFilter):
            raise TypeError("filter must be a RowFilter, or a sequence of RowFilter / None with one entry per query")
    arr = (C.c_void_p * nq)(*[f._h if f is not None else None for f in fs])
    arr._keep = fs
    return arr


def filtered_plan(n_rows, allowed, search_list, dedup_on=False):
    """What regime="auto" does for a filter of `allowed` rows on a graph of `n_rows` (mse_filtered_plan): (regime name, effective
    search_list).  No allowed row: "list" (all padding).  L' = ceil(search_list * n_rows / allowed) <= 1024: "graph" at max(search_list,
    L'); otherwise "list" -- or "graph" at 1024 with the de-duplication on."""
    rg, eff = C.c_int(), C.c_size_t()
    check(ffi.lib().mse_filtered_plan(int(n_rows), int(allowed), int(search_list), int(bool(dedup_on)), C.byref(rg), C.byref(eff)),
          "filtered_plan")
    return _REGIME_NAMES[rg.value], int(eff.value)


def disk_search_batch(searcher: Searcher, quantizer, codes, dgraph: DeviceGraph, starts, queries, luts=None, descriptor_scales=None,
                      disable_pq=False, beamwidth=1, search_list=1000, visited_cap=4096, as_arrays=False, filter=None):
    """query_disk_index::greedy_search for a batch of queries, entirely on the device (one workgroup per query).
    filter (a RowFilter, f16 queries only): the same traversal, but a fetched node enters the visited list only if the filter allows
    it (and it has a url) -- the search over an index whose has_url is has_url AND allowed.  A sequence of nq RowFilter / None gives
    every query its own filter (None: unfiltered) in the same single launch (mse_disk_search_batch_filtered_each).
    as_arrays=True returns the padded output arrays themselves (dict: buf_ids, buf_scores, buf_len, visited_ids,
    visited_scores, n_visited, cmps, pq_cmps) instead of one tuple per query.
    queries: f16 rows with `luts` (QueryLUTs / [nq][64*256] f32; not needed with disable_pq), or f32 rows with luts=None --
    then the f16 copies and the tables are made on the device (query_disk_index.rs:475-477).
    Returns a list of (buffer ids, buffer scores, visited ids, visited scores, cmps, pq_cmps)."""
    qa = np.asarray(queries)
    from_f32 = qa.dtype == np.float32 and luts is None
    if from_f32:
        q = np.ascontiguousarray(qa.reshape(-1, qa.shape[-1]), np.float32)
    else:
        q = _bits(queries)
        q = q.reshape(-1, q.shape[-1])
    nq = q.shape[0]
    tables = None
    if not from_f32 and luts is not None:
        tables = np.ascontiguousarray(np.stack([getattr(t, "table", t) for t in luts]) if not isinstance(luts, np.ndarray) else luts,
                                      np.float32).reshape(nq, -1)
    st = np.ascontiguousarray(starts, np.uint32).reshape(nq)
    sc = None
    if descriptor_scales is not None:
        sc = np.ascontiguousarray(descriptor_scales, np.float32)
        if sc.ndim == 1:
            sc = np.ascontiguousarray(np.broadcast_to(sc, (nq, sc.size)))
    bi, bs, bl = np.empty((nq, search_list), np.uint32), np.empty((nq, search_list), np.int64), np.empty(nq, np.uint32)
    vi, vs = np.empty((nq, visited_cap), np.uint32), np.empty((nq, visited_cap), np.int64)
    nv, cm, pc = np.empty(nq, np.uint32), np.empty(nq, np.uint32), np.empty(nq, np.uint32)
    tail = (nq, int(bool(disable_pq)), int(beamwidth), int(search_list), _p(bi, C.c_uint32), _p(bs, C.c_int64), _p(bl, C.c_uint32),
            _p(vi, C.c_uint32), _p(vs, C.c_int64), visited_cap, _p(nv, C.c_uint32), _p(cm, C.c_uint32), _p(pc, C.c_uint32))
    scp = _p(sc, C.c_float) if sc is not None else None
    each = _filter_array(filter, nq)
    if each is not None:
        if from_f32:
            raise MseError("disk_search_batch: a filtered search takes f16 queries (with luts, or disable_pq)")
        check(ffi.lib().mse_disk_search_batch_filtered_each(searcher._h, quantizer._h if quantizer is not None else None,
                                                            codes._h if codes is not None else None, dgraph._h, each, _p(st, C.c_uint32),
                                                            _p(q, C.c_uint16), _p(tables, C.c_float) if tables is not None else None, scp, *tail),
              "disk_search_batch_filtered_each")
    elif filter is not None:
        if from_f32:
            raise MseError("disk_search_batch: a filtered search takes f16 queries (with luts, or disable_pq)")
        check(ffi.lib().mse_disk_search_batch_filtered(searcher._h, quantizer._h if quantizer is not None else None,
                                                       codes._h if codes is not None else None, dgraph._h, filter._h, _p(st, C.c_uint32),
                                                       _p(q, C.c_uint16), _p(tables, C.c_float) if tables is not None else None, scp, *tail),
              "disk_search_batch_filtered")
    elif from_f32:
        check(ffi.lib().mse_disk_search_batch_f32(searcher._h, quantizer._h if quantizer is not None else None,
                                                  codes._h if codes is not None else None, dgraph._h, _p(st, C.c_uint32), _p(q, C.c_float),
                                                  scp, *tail), "disk_search_batch_f32")
    else:
        check(ffi.lib().mse_disk_search_batch(searcher._h, quantizer._h if quantizer is not None else None,
                                              codes._h if codes is not None else None, dgraph._h, _p(st, C.c_uint32), _p(q, C.c_uint16),
                                              _p(tables, C.c_float) if tables is not None else None, scp, *tail), "disk_search_batch")
    if as_arrays:
        return {"buf_ids": bi, "buf_scores": bs, "buf_len": bl, "visited_ids": vi, "visited_scores": vs, "n_visited": nv, "cmps": cm,
                "pq_cmps": pc}
    if int(nv.max(initial=0)) > visited_cap:
        # the reference keeps every visited record (query_disk_index.rs:168-186); a silently shortened list would change results
        raise MseError(f"a search visited {int(nv.max())} records but visited_cap is {visited_cap}: raise visited_cap "
                       "(as_arrays=True returns the truncated arrays together with n_visited instead)")
    out = []
    for i in range(nq):
        k = min(int(nv[i]), visited_cap)
        out.append((bi[i, :bl[i]].copy(), bs[i, :bl[i]].copy(), vi[i, :k].copy(), vs[i, :k].copy(), int(cm[i]), int(pc[i])))
    return out


def set_entries(dgraph, vecs, node_ids):
    """The entry table of disk_query_topk: `node_ids` name the entry records (the reference: the shard medioids,
    query_disk_index.rs:254-256,447-450; for a one-piece index a sample of its rows); copies of their vectors stay with the graph."""
    ids = np.ascontiguousarray(node_ids, np.uint32).reshape(-1)
    check(ffi.lib().mse_graph_set_entries(dgraph._h, vecs._h, _p(ids, C.c_uint32), ids.size), "graph_set_entries")


def set_entry_centroids(dgraph, centroids, medioid_ids):
    """The reference's own entry rule (query_disk_index.rs:254-256,447-450): `centroids` [n_shards, d] f32 are the shard centroids of
    the index header, `medioid_ids` the shards' start nodes; a search starts at the medioid of the shard whose centroid has the largest
    scale_dot_result_f64(dot(centroid, query)), last maximum on ties."""
    c = np.ascontiguousarray(centroids, np.float32)
    ids = np.ascontiguousarray(medioid_ids, np.uint32).reshape(-1)
    if c.ndim != 2 or c.shape[0] != ids.size:
        raise MseError("centroids must be [n_shards, d] with one medioid id per shard")
    check(ffi.lib().mse_graph_set_entry_centroids(dgraph._h, _p(c, C.c_float), c.shape[1], _p(ids, C.c_uint32), ids.size),
          "graph_set_entry_centroids")


def set_dedup(dgraph, threshold=DUPLICATES_THRESHOLD):
    """The handler's runtime de-duplication (query_disk_index.rs:482-527) inside disk_query_topk: visited records that resemble an
    already kept one (dot above `threshold`, visit order) leave the list before it is ordered.  0 switches it off (the default)."""
    check(ffi.lib().mse_graph_set_dedup(dgraph._h, float(threshold)), "graph_set_dedup")


def set_coalescer(dgraph, max_queries_per_pass=0, max_wait_us=0, workers=0):
    """How the graph's coalescer serves small request-path calls from many threads (0 = the defaults: 1024, 200 us, 3 workers)."""
    check(ffi.lib().mse_graph_set_coalescer(dgraph._h, int(max_queries_per_pass), int(max_wait_us), int(workers)), "graph_set_coalescer")


def coalescer_stats(dgraph):
    out = (C.c_uint64 * 6)()
    check(ffi.lib().mse_graph_coalescer_stats(dgraph._h, out), "graph_coalescer_stats")
    return {"queries": int(out[0]), "requests": int(out[1]), "passes": int(out[2]), "max_pass_queries": int(out[3]),
            "deadline_fires": int(out[4]), "run_us": int(out[5])}


def coalescer_groups(dgraph):
    """What shared a launch (mse_graph_coalescer_groups): the groups of coalesced requests that ran as one launch each, and the requests
    in them.  groups == requests: nothing shared."""
    out = (C.c_uint64 * 2)()
    check(ffi.lib().mse_graph_coalescer_groups(dgraph._h, out), "graph_coalescer_groups")
    return {"groups": int(out[0]), "requests": int(out[1])}


def disk_query_topk(searcher: Searcher, quantizer, codes, dgraph, queries, k, starts=None, luts=None, descriptor_scales=None,
                    disable_pq=False, beamwidth=1, search_list=1000, filter=None, regime="auto", groups=None):
    """The request path of query_disk_index (:436-540) for a batch in one device submission: entry node (by the graph's entry table
    when `starts` is None), greedy_search, the visited records ordered by exact score and cut to the first k.  f16 query rows in
    (a host array, or `(device_pointer, nq)` for rows already on the device),
    (ids [nq, k] uint32, scores [nq, k] int64, stats dict) out; ids / scores equal topk_of_visited(disk_search_batch(...)) for the
    same start nodes.  Rows with fewer than k visited records are padded with ID_NONE / INT64_MIN.
    filter (a RowFilter): only rows it allows (and that have a url) are returned.  regime "graph": the same traversal at search_list,
    disallowed nodes walked through but not returned; "list": the exact k best of the eligible rows, no traversal (n_visited = cmps =
    eligible rows); "auto": whichever filtered_plan(len(graph), filter.count, search_list, dedup on) names, at its search_list.
    A sequence of nq RowFilter / None gives every query its own filter (None: unfiltered; mse_disk_query_topk_filtered_each): row i is
    the answer of the one-query call with filter[i], the regime resolved per query, and queries that can share a launch do.
    groups (a RowGroups, by row id): one result per group -- of the records this search visited, ranked as above, the first of every
    group; fewer than k groups among them show as padding (ask again with a longer search_list).  With or without a filter."""
    from_f32 = False
    if isinstance(queries, tuple):      # (device pointer, nq): f16 rows already resident on the searcher's device, contiguous
        q_ptr, nq = C.cast(C.c_void_p(int(queries[0])), C.POINTER(C.c_uint16)), int(queries[1])
    elif np.asarray(queries).dtype == np.float32 and luts is None:
        # f32 rows in, as the reference's handler gets them (:436-477): f16 copies and distance tables are made on the device
        from_f32 = True
        q = np.ascontiguousarray(np.asarray(queries).reshape(-1, np.asarray(queries).shape[-1]), np.float32)
        nq = q.shape[0]
        q_ptr = _p(q, C.c_float)
    else:
        q = _bits(queries)
        q = q.reshape(-1, q.shape[-1])
        nq = q.shape[0]
        q_ptr = _p(q, C.c_uint16)
    tables = None
    if luts is not None:
        tables = np.ascontiguousarray(np.stack([getattr(t, "table", t) for t in luts]) if not isinstance(luts, np.ndarray) else luts,
                                      np.float32).reshape(nq, -1)
    st = None if starts is None else np.ascontiguousarray(starts, np.uint32).reshape(nq)
    sc = None
    if descriptor_scales is not None:
        sc = np.ascontiguousarray(descriptor_scales, np.float32)
        if sc.ndim == 1:
            sc = np.ascontiguousarray(np.broadcast_to(sc, (nq, sc.size)))
    ids, scores = np.empty((nq, k), np.uint32), np.empty((nq, k), np.int64)
    nv, cm, pc = np.empty(nq, np.uint32), np.empty(nq, np.uint32), np.empty(nq, np.uint32)
    tail = (nq, int(bool(disable_pq)), int(beamwidth), int(search_list), int(k), _p(ids, C.c_uint32), _p(scores, C.c_int64), _p(nv, C.c_uint32),
            _p(cm, C.c_uint32), _p(pc, C.c_uint32))
    head = (searcher._h, quantizer._h if quantizer is not None else None, codes._h if codes is not None else None, dgraph._h,
            _p(st, C.c_uint32) if st is not None else None, q_ptr)
    scp = _p(sc, C.c_float) if sc is not None else None
    each = _filter_array(filter, nq)
    if each is not None:
        ehead = head[:4] + (each, _regime(regime), groups._h if groups is not None else None) + head[4:]
        if from_f32:
            check(ffi.lib().mse_disk_query_topk_filtered_each_f32(*ehead, scp, *tail), "disk_query_topk_filtered_each_f32")
        else:
            check(ffi.lib().mse_disk_query_topk_filtered_each(*ehead, _p(tables, C.c_float) if tables is not None else None, scp, *tail),
                  "disk_query_topk_filtered_each")
    elif groups is not None:
        ghead = head[:4] + (groups._h, filter._h if filter is not None else None, _regime(regime)) + head[4:]
        if from_f32:
            check(ffi.lib().mse_disk_query_topk_grouped_f32(*ghead, scp, *tail), "disk_query_topk_grouped_f32")
        else:
            check(ffi.lib().mse_disk_query_topk_grouped(*ghead, _p(tables, C.c_float) if tables is not None else None, scp, *tail),
                  "disk_query_topk_grouped")
    elif filter is not None:
        fhead = head[:4] + (filter._h, _regime(regime)) + head[4:]
        if from_f32:
            check(ffi.lib().mse_disk_query_topk_filtered_f32(*fhead, scp, *tail), "disk_query_topk_filtered_f32")
        else:
            check(ffi.lib().mse_disk_query_topk_filtered(*fhead, _p(tables, C.c_float) if tables is not None else None, scp, *tail),
                  "disk_query_topk_filtered")
    elif from_f32:
        check(ffi.lib().mse_disk_query_topk_f32(*head, scp, *tail), "disk_query_topk_f32")
    else:
        check(ffi.lib().mse_disk_query_topk(*head, _p(tables, C.c_float) if tables is not None else None, scp, *tail), "disk_query_topk")
    return ids, scores, {"n_visited": nv, "cmps": cm, "pq_cmps": pc}


_OWN_FILTER = object()   # QueryTickets.submit: "the filter this object was made with"


class QueryTickets:
    """The request path without a thread per request (include/mse.h "WITHOUT A THREAD PER REQUEST"): one host thread keeps many
    one-query requests of a graph in flight, the way the reference's monoio tasks would (src/query_disk_index.rs:640-655,716-732).
    submit() queues a request and returns its key; collect() hands back requests executed since, as (key, ids [nq, k], scores
    [nq, k]) -- the answers of disk_query_topk for the same queries, bit for bit.  By default a graph has ONE completion list:
    collect() of any such QueryTickets object of that graph returns whatever has completed, whichever object (search settings)
    submitted it (the output arrays of requests in flight are kept alive on the graph object); with own_queue=True the object has a
    completion queue of its own."""

    def __init__(self, searcher: Searcher, quantizer, codes, dgraph, k, disable_pq=False, beamwidth=1, search_list=1000, own_queue=False,
                 filter=None, regime="auto", groups=None):
        """own_queue=True: a completion queue of this object's own (mse_completion_queue_*): its requests come back through its
        collect() / fileno() and nowhere else -- one per event loop of a host that runs several.
        filter / regime / groups: as disk_query_topk; filter and grouping are kept alive by this object (copy=False is for requests
        with neither)."""
        import threading
        self._filter, self._regime, self._groups = filter, _regime(regime), groups
        self._s, self._pq, self._codes, self._g = searcher, quantizer, codes, dgraph
        self.k, self.disable_pq, self.beamwidth, self.search_list = int(k), bool(disable_pq), int(beamwidth), int(search_list)
        self._q = None
        if own_queue:
            self._q = check_ptr(ffi.lib().mse_completion_queue_new(), "mse_completion_queue_new")
            self._reg = {"lock": threading.Lock(), "next": 1, "out": {}}
        else:
            if not hasattr(dgraph, "_tickets"):
                dgraph._tickets = {"lock": threading.Lock(), "next": 1, "out": {}}
            self._reg = dgraph._tickets

    def close(self):
        """Release the object's own completion queue (no request of it may be in flight)."""
        if getattr(self, "_q", None):
            if self._reg["out"]:
                raise MseError("completion queue closed with requests in flight")
            ffi.lib().mse_completion_queue_free(self._q)
            self._q = None

    def __del__(self):
        try:
            if getattr(self, "_q", None) and not self._reg["out"]:
                ffi.lib().mse_completion_queue_free(self._q)
                self._q = None
        except Exception:  # noqa: BLE001
            pass

    @property
    def in_flight(self):
        """Requests of the whole graph submitted and not yet collected."""
        return len(self._reg["out"])

    def submit(self, query_f32, descriptor_scales=None, key=None, copy=True, filter=_OWN_FILTER):
        """copy=False: the library reads the query where it lies (mse_disk_query_submit_f32_nocopy); this object keeps the array alive
        until the request has been collected.
        filter: a RowFilter for THIS request in place of the object's own (None: this request is unfiltered); it is kept alive until
        the request has been collected.  Requests with different filters still share a launch when they resolve to the graph regime
        at the same search_list."""
        flt_obj = self._filter if filter is _OWN_FILTER else filter
        if flt_obj is not None and not isinstance(flt_obj, RowFilter):
            raise TypeError("filter must be a RowFilter or None")
        q = np.ascontiguousarray(np.asarray(query_f32, np.float32).reshape(-1, np.asarray(query_f32).shape[-1]))
        nq = q.shape[0]
        sc = None
        if descriptor_scales is not None:
            sc = np.asarray(descriptor_scales, np.float32)
            sc = np.ascontiguousarray(np.broadcast_to(sc, (nq, sc.shape[-1])))
        ids, scores = np.empty((nq, self.k), np.uint32), np.empty((nq, self.k), np.int64)
        with self._reg["lock"]:
            tag = self._reg["next"]
            self._reg["next"] += 1
            self._reg["out"][tag] = (key if key is not None else tag, ids, scores, flt_obj) + (() if copy else (q, sc))   # before the request can complete
        t = C.c_void_p()
        try:
            if (flt_obj is not None or self._groups is not None) and not copy:
                raise MseError("QueryTickets: copy=False is not available with a filter or a grouping")
            fn = ffi.lib().mse_disk_query_submit_f32 if copy else ffi.lib().mse_disk_query_submit_f32_nocopy
            flt = ()
            if flt_obj is not None:
                fn, flt = ffi.lib().mse_disk_query_submit_filtered_f32, (flt_obj._h, self._regime)
            if self._groups is not None:
                fn = ffi.lib().mse_disk_query_submit_grouped_f32
                flt = (self._groups._h, flt_obj._h if flt_obj is not None else None, self._regime)
            check(fn(self._s._h, self._pq._h if self._pq is not None else None,
                                                      self._codes._h if self._codes is not None else None, self._g._h, *flt, _p(q, C.c_float),
                                                      _p(sc, C.c_float) if sc is not None else None, nq, int(self.disable_pq), self.beamwidth,
                                                      self.search_list, self.k, _p(ids, C.c_uint32), _p(scores, C.c_int64), None, None, None,
                                                      C.c_void_p(tag), self._q, C.byref(t)), "disk_query_submit_f32")
        except MseError:
            with self._reg["lock"]:
                self._reg["out"].pop(tag, None)
            raise
        return key if key is not None else tag

    def fileno(self):
        """An eventfd that becomes readable when requests of the graph have completed (for select / epoll / asyncio's add_reader):
        read its 8-byte counter, then collect(timeout_us=0) until it returns []."""
        fd = ffi.lib().mse_completion_queue_fd(self._q) if self._q else ffi.lib().mse_graph_completion_fd(self._g._h)
        if fd < 0:
            check(-1, "completion fd")
        return fd

    def collect(self, max_tickets=256, timeout_us=-1):
        """Executed requests of the graph, in completion order: [(key, ids, scores)].  Sleeps up to timeout_us for the first (0: poll,
        < 0: until one is there); [] if none came in time.  A request that failed when executed raises MseError with its own
        message once the successful ones of the same call have been returned (they are handed out first, the failure on the next
        call)."""
        pending = self._reg.setdefault("failed", [])
        if pending:
            raise pending.pop(0)
        buf = (C.c_void_p * int(max_tickets))()
        if self._q:
            n = ffi.lib().mse_completion_queue_wait(self._q, buf, int(max_tickets), int(timeout_us))
        else:
            n = ffi.lib().mse_graph_completions(self._g._h, buf, int(max_tickets), int(timeout_us))
        if n < 0:
            check(-1, "completions")
        done = []
        for i in range(n):
            t = buf[i]
            tag = int(ffi.lib().mse_ticket_user(t) or 0)
            rc = ffi.lib().mse_ticket_status(t)
            msg = ffi.lib().mse_ticket_error(t).decode() if rc else ""
            ffi.lib().mse_ticket_free(t)
            with self._reg["lock"]:
                key, ids, scores = self._reg["out"].pop(tag)[:3]
            if rc:
                pending.append(MseError(f"request {key!r}: {msg or 'search failed'}"))
            else:
                done.append((key, ids, scores))
        if not done and pending:
            raise pending.pop(0)
        return done


def topk_of_visited(res, k, keep=None):
    """Batch form of the server's last step (query_disk_index.rs:529-540): the reference sorts the WHOLE visited list by exact
    score after the dedup filter (:482-527) and returns all of it; this helper cuts that sorted list to its first k ids per query
    (stable order), from disk_search_batch(..., as_arrays=True).  `keep` ([nq, visited_cap] bool, e.g. from dedup_visited per
    query) drops filtered records first; without it no dedup is applied.  Always returns [nq, k]: rows with fewer than k
    records are padded with ID_NONE.  Raises if a search visited more records than visited_cap held (the reference keeps all)."""
    vi, vs, nv = res["visited_ids"], res["visited_scores"], res["n_visited"]
    cap = vi.shape[1]
    if int(nv.max(initial=0)) > cap:
        raise ValueError(f"a search visited {int(nv.max())} records but visited_cap is {cap}: raise visited_cap (the reference keeps every visited record)")
    nq = vi.shape[0]
    w = int(min(cap, max(int(nv.max(initial=0)), 1)))
    lowest = np.iinfo(np.int64).min
    sc = vs[:, :w].copy()
    dead = np.arange(w)[None, :] >= nv[:, None]
    if keep is not None:
        dead |= ~np.asarray(keep, bool)[:, :w]
    sc[dead] = lowest
    # two stable passes: order by score descending without the precision loss of a float cast
    order = np.argsort(-(sc >> 1), axis=1, kind="stable")          # coarse (halved scores cannot overflow when negated)
    fine = np.take_along_axis(sc, order, axis=1)
    fix = np.lexsort((np.arange(w)[None, :].repeat(nq, 0), -(fine & 1), -(fine >> 1)), axis=1)
    order = np.take_along_axis(order, fix, axis=1)
    ids = np.full((nq, k), 0xFFFFFFFF, np.int64)
    m = min(k, w)
    top = order[:, :m]
    ids[:, :m] = np.take_along_axis(vi[:, :w], top, axis=1)
    ids[:, :m][np.take_along_axis(dead, top, axis=1)] = 0xFFFFFFFF
    return ids


def greedy_search(searcher: Searcher, start, base_vectors_only, query, graph: IndexGraph, l,
                  query_breakpoint=0xFFFFFFFF):
    """lib.rs:183-211.  Returns (NeighbourBuffer, distances); results are buffer.ids, best first."""
    q = _bits(query).reshape(-1)
    buf = NeighbourBuffer(l)
    nd = C.c_size_t()
    check(ffi.lib().mse_greedy_search(searcher._h, _p(graph.adj, C.c_uint32), _p(graph.deg, C.c_uint32),
                                      graph.adj.shape[1], int(start), _p(q, C.c_uint16), int(bool(base_vectors_only)),
                                      int(query_breakpoint), buf._h, C.byref(nd)), "greedy_search")
    return buf, int(nd.value)


# ---- Vamana graph build on the device (diskann/src/lib.rs:213-389; src/generate_index_shard.rs:85-133) -------------

def IndexBuildConfig(r=64, l=192, maxc=750, alpha=65536, query_alpha=65536, saturate_graph=False, query_breakpoint=0xFFFFFFFF,
                     max_add_per_stitch_iter=16):
    """IndexBuildConfig (lib.rs:42-52) with generate_index_shard's defaults (:22-33,85-94)."""
    return ffi.BuildConfig(r, l, maxc, alpha, query_alpha, int(bool(saturate_graph)), query_breakpoint, max_add_per_stitch_iter)


class BuildGraph(_RowDeletes):
    """The graph under construction, resident in HBM (IndexGraph::empty + the build passes)."""

    def __init__(self, n, r, graph: IndexGraph = None):
        if graph is not None:
            assert graph.adj.shape == (n, r)
            self._h = check_ptr(ffi.lib().mse_graph_from_host(_p(graph.adj, C.c_uint32), _p(graph.deg, C.c_uint32), n, r, None),
                                "mse_graph_from_host")
        else:
            self._h = check_ptr(ffi.lib().mse_graph_new(n, r), "mse_graph_new")
        self.n, self.r = n, r

    def random_fill(self, seed, r=None):
        """random_fill_graph (lib.rs:376-389) from a counter-based generator (a seed names one graph)."""
        check(ffi.lib().mse_graph_random_fill(self._h, int(seed), self.r if r is None else r), "graph_random_fill")

    def build(self, searcher: Searcher, order, medioid, config, batch=1024):
        """build_graph (lib.rs:287-324); `order` = the shuffled point ids (sigmas); batch = 1 is the sequential form."""
        o = np.ascontiguousarray(order, np.uint32)
        check(ffi.lib().mse_build_graph(searcher._h, self._h, _p(o, C.c_uint32), o.size, int(batch), int(medioid), C.byref(config)),
              "build_graph")

    def robust_stitch(self, searcher: Searcher, queries_order, config):
        """robust_stitch (lib.rs:326-374)."""
        o = np.ascontiguousarray(queries_order, np.uint32)
        check(ffi.lib().mse_robust_stitch(searcher._h, self._h, _p(o, C.c_uint32), C.byref(config)), "robust_stitch")

    def to_host(self) -> IndexGraph:
        adj, deg = np.empty((self.n, self.r), np.uint32), np.empty(self.n, np.uint32)
        check(ffi.lib().mse_graph_to_host(self._h, _p(adj, C.c_uint32), _p(deg, C.c_uint32)), "graph_to_host")
        return IndexGraph(adj, deg)

    def search_batch(self, searcher: Searcher, starts, queries, l, base_vectors_only=False, query_breakpoint=0xFFFFFFFF, as_arrays=False):
        """diskann::greedy_search (lib.rs:183-211) for a batch of queries on the device: list of (ids, scores, distances), or with
        as_arrays=True the padded arrays (ids [nq][l], scores [nq][l], len [nq], distances [nq])."""
        q = _bits(queries)
        q = q.reshape(-1, q.shape[-1])
        nq = q.shape[0]
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(starts, np.uint32), (nq,)))
        bi, bs = np.empty((nq, l), np.uint32), np.empty((nq, l), np.int64)
        bl, nd = np.empty(nq, np.uint32), np.empty(nq, np.uint32)
        check(ffi.lib().mse_graph_search_batch(searcher._h, self._h, _p(st, C.c_uint32), _p(q, C.c_uint16), nq, int(l),
                                               int(bool(base_vectors_only)), int(query_breakpoint), _p(bi, C.c_uint32),
                                               _p(bs, C.c_int64), _p(bl, C.c_uint32), _p(nd, C.c_uint32)), "graph_search_batch")
        if as_arrays:
            return bi, bs, bl, nd
        return [(bi[i, :bl[i]].copy(), bs[i, :bl[i]].copy(), int(nd[i])) for i in range(nq)]

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_graph_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def robust_prune(searcher: Searcher, cand_ids, cand_scores, p, config):
    """robust_prune (lib.rs:227-285) on a candidate list; returns the new neighbour list."""
    ci, cs = np.ascontiguousarray(cand_ids, np.uint32), np.ascontiguousarray(cand_scores, np.int64)
    out = np.empty(int(config.r), np.uint32)
    nn = C.c_size_t()
    check(ffi.lib().mse_robust_prune(searcher._h, _p(ci, C.c_uint32), _p(cs, C.c_int64), ci.size, int(p), C.byref(config),
                                     _p(out, C.c_uint32), C.byref(nn)), "robust_prune")
    return out[:nn.value].copy()
