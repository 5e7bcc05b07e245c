"""Grouped graph search on the device (include/mse.h "grouped graph search"), bit for bit: the group step alone over caller-supplied
visited lists (mse_debug_visited_collapse, both table forms) against the numpy restatement of tests/grouped_graph_ref.py, and the request
path against the collapse of the CPU oracle's visited lists -- every parameter of the traversal, both kinds of graph, both entry rules,
the de-duplication, the query forms, the three filter regimes, shared submissions, one handle across calls, and argument errors."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import SEED_CENTRES
from grouped_graph_ref import group_step, grouped_cut
from grouped_ref import GROUP_NONE, I64_MIN, ID_NONE, grouped_topk
from test_gpu_filtered_graph import N, SCALES, Index, clustered_rows, sorted_cut

pytestmark = pytest.mark.gpu
K = 10
I64_MAX = np.iinfo(np.int64).max
COUNTERS = ("n_visited", "cmps", "pq_cmps")


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------------------
ID_SPACE, G_LEN = 60000, 40000            # ids are drawn below ID_SPACE; the grouping speaks for the first G_LEN rows only
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 2048, 2049, 3000]   # at cap 2112: 3000 is clamped to the cap
# (cap, n_visited of every query of the launch): nq of 1, 3 and 70, different lengths in one launch; 4096 at cap 4096 is the longest
# list of the LDS table, cap 8448 takes the table in global memory -- 70 queries there are more than one chunk of its byte budget
LAUNCHES = {
    "one-257": (2112, [257]),
    "three-mixed": (2112, [0, 65, 2049]),
    "seventy-every-length": (2112, [LENGTHS[q % len(LENGTHS)] for q in range(70)]),
    "cap4096": (4096, [4096, 1, 4095]),
    "cap8448": (8448, [8448, 300, 8447]),
    "cap8448-seventy": (8448, [(8448, 0, 1, 64, 257, 700, 2049)[q % 7] for q in range(70)]),
}


def table_bits(n):
    """the kernel's table for a list of n records: the power of two of at least 2 n slots, 64 at least (group.hip visited_group_kernel)"""
    bits = 6
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


def kernel_hash(g, bits):
    """the kernel's first probe for group g: its multiplicative hash (group.hip visited_group_body)"""
    return ((int(g) * 2654435761) & 0xFFFFFFFF) >> (32 - bits)


def make_grouping(kind, rng):
    if kind == "one":
        return np.full(G_LEN, 7, np.uint32)
    if kind == "none":
        return np.full(G_LEN, GROUP_NONE, np.uint32)
    if kind == "distinct":
        return np.arange(G_LEN, dtype=np.uint32)
    if kind == "collide":
        # group ids whose first probe is ONE slot of the 512-slot table of a 255 / 256-record list, derived from the kernel's hash: every
        # insert after the first walks the probe chain (in longer lists' larger tables the same ids still cluster in a few slots)
        bits = table_bits(256)
        same = [g for g in range(G_LEN) if kernel_hash(g, bits) == kernel_hash(12345, bits)]
        assert len(same) >= 40 and table_bits(255) == bits
        return np.array(same, np.uint32)[rng.integers(0, len(same), G_LEN)]
    g = rng.integers(0, 300, G_LEN).astype(np.uint32)           # "random": a few hundred groups, a third of the rows NONE
    g[rng.random(G_LEN) < 0.3] = GROUP_NONE
    return g


def make_lists(cap, lengths, group_of, rng):
    """Lists in the request path's layout.  Score kinds rotate over the queries: equal within a group (the lowest id stays), negative and
    positive mixed, INT64_MIN / INT64_MAX, many ties; holes in the middle as the de-duplication leaves them; ids at or past the
    grouping; past n_visited live-looking grouped records that must stay as they are."""
    nq = len(lengths)
    ids = np.empty((nq, cap), np.uint32)
    sc = np.empty((nq, cap), np.int64)
    for q in range(nq):
        ids[q] = rng.choice(ID_SPACE, cap, replace=False)
        kind = q % 4
        if kind == 0:
            inside = ids[q] < G_LEN
            g = np.where(inside, group_of[np.minimum(ids[q], G_LEN - 1)], GROUP_NONE).astype(np.int64)
            sc[q] = (g % 1000) * 77 - 5000
        elif kind == 1:
            sc[q] = rng.integers(-(1 << 40), 1 << 40, cap)
        elif kind == 2:
            sc[q] = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1], np.int64), cap)
        else:
            sc[q] = rng.integers(-3, 4, cap)
        n = min(lengths[q], cap)
        hole = np.flatnonzero(rng.random(n) < 0.1)
        ids[q, hole], sc[q, hole] = ID_NONE, I64_MIN
    return ids, sc


def run_hook(mse, searcher, groups, ids, sc, lengths):
    from mse import ffi
    ids, sc = np.ascontiguousarray(ids.copy()), np.ascontiguousarray(sc.copy())
    nv = np.ascontiguousarray(lengths, np.uint32)
    ffi.check(ffi.lib().mse_debug_visited_collapse(searcher._h, groups._h, ids.ctypes.data_as(ffi.u32p), sc.ctypes.data_as(ffi.i64p), ids.shape[1],
                                                   nv.ctypes.data_as(ffi.u32p), ids.shape[0]), "mse_debug_visited_collapse")
    return ids, sc


@pytest.fixture(scope="module")
def hook_searcher(gpu, mse, orc):
    return mse.Searcher(mse.VectorList.from_f16s(orc.gen_rows_f16(3, 0, 64), 1152))


@pytest.mark.parametrize("kind", ["one", "none", "distinct", "collide", "random"])
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_group_step_alone_equals_the_numpy_restatement(hook_searcher, mse, launch, kind):
    cap, lengths = LAUNCHES[launch]
    rng = np.random.default_rng(len(launch) * 131 + len(kind))
    group_of = make_grouping(kind, rng)
    ids, sc = make_lists(cap, lengths, group_of, rng)
    groups = mse.RowGroups(group_of)
    got_i, got_s = run_hook(mse, hook_searcher, groups, ids, sc, lengths)
    removed = 0
    for q, n_vis in enumerate(lengths):
        want_i, want_s = group_step(ids[q], sc[q], n_vis, group_of)
        assert np.array_equal(got_i[q], want_i) and np.array_equal(got_s[q], want_s), (launch, kind, q)
        n = min(n_vis, cap)
        gone = got_i[q] != ids[q]
        # removed records are exactly (ID_NONE, INT64_MIN); survivors are unchanged and in place; entries at or past n are untouched
        assert np.all(got_i[q][gone] == ID_NONE) and np.all(got_s[q][gone] == I64_MIN)
        assert np.array_equal(got_s[q][~gone], sc[q][~gone]) and not gone[n:].any() and np.array_equal(got_s[q][n:], sc[q][n:])
        removed += int(gone.sum())
        if kind == "one" and n:
            inside = np.flatnonzero((ids[q][:n] != ID_NONE) & (ids[q][:n] < G_LEN))
            assert (got_i[q][inside] != ID_NONE).sum() == min(1, inside.size)
    assert (removed == 0) == (kind in ("none", "distinct")), removed


# ---- the request path ---------------------------------------------------------------------------------------------------------------------
class Grouped(Index):
    """The 20 000-row index of tests/test_gpu_filtered_graph.py with an entry table on both graphs and the issue's groupings."""

    def __init__(self, mse, orc, d, seed):
        super().__init__(mse, orc, d, seed)
        rng = np.random.default_rng(seed + 7)
        self.entry_ids = np.sort(rng.choice(N, 40, replace=False)).astype(np.uint32)
        for g in self.graphs.values():
            mse.set_entries(g, self.vecs, self.entry_ids)
        _, best = orc.bruteforce_topk(self.base[self.entry_ids], self.qh, 1)
        self.by_table = self.entry_ids[best[:, 0]]
        centres = orc.f16_to_f32(orc.gen_rows_f16(SEED_CENTRES, 0, 48))[:, :d]
        centres = centres / np.linalg.norm(centres, axis=1, keepdims=True)
        half = (np.arange(N, dtype=np.uint32) // 8) * 8
        half[rng.random(N) < 0.5] = GROUP_NONE
        self.groupings = {
            "runs8": (np.arange(N, dtype=np.uint32) // 8) * 8,                       # runs of 8 rows, named by their first row
            "cluster": np.argmax(self.x @ centres.T, axis=1).astype(np.uint32),      # the rows' cluster centre: 48 large groups
            "half-none": half,
            "short": ((np.arange(N - 3333, dtype=np.uint32) // 8) * 8),              # shorter than the graph
            "none": np.full(N, GROUP_NONE, np.uint32),
        }


@pytest.fixture(scope="module")
def big(gpu, mse, orc):
    return Grouped(mse, orc, 1152, 31)


def fit_grouping(name, group_of, lists):
    """The seeded grouping, or -- where it misses a condition the test sets on its inputs -- one built from the oracle's visited lists:
    `differs` (every grouping but all-NONE): some query's grouped answer differs from its ungrouped one; else the three best records of
    every query that lie inside the grouping share a group.  `padded` (cluster): some query comes back short; else every visited record of
    the first query shares a group.  Returns the grouping; the conditions themselves are asserted by the caller."""
    g = group_of.copy()

    def answers(gr):
        return [(grouped_cut(vi, vs, gr, K), sorted_cut(vi, vs, K)) for vi, vs in lists]

    if name != "none" and not any(not np.array_equal(a[0], b[0]) for a, b in answers(g)):
        for vi, vs in lists:
            inside = [int(r) for r in sorted_cut(vi, vs, len(vi))[0] if r < len(g)][:3]
            g[inside] = min(inside)
    if name == "cluster" and not any((a[0] == ID_NONE).any() for a, _ in answers(g)):
        vi = lists[0][0]
        g[vi[vi < len(g)]] = int(vi.min())
    return g


def check_conditions(name, group_of, lists):
    ans = [(grouped_cut(vi, vs, group_of, K), sorted_cut(vi, vs, K)) for vi, vs in lists]
    if name == "none":
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in ans)
    else:
        assert any(not np.array_equal(a[0], b[0]) for a, b in ans), "no query's grouped answer differs from its ungrouped answer"
    if name == "cluster":
        assert any((a[0] == ID_NONE).any() for a, _ in ans), "no query comes back with padding under the cluster grouping"
    if name == "runs8":
        assert any((a[0] != ID_NONE).all() for a, _ in ans), "no query fills all k under runs of 8"


GROUPINGS = ["runs8", "cluster", "half-none", "short", "none"]
GRID = [(b, dp, sc, L) for b in (1, 4, 8) for dp in (False, True) for sc in (True, False) for L in (12, 200, 1024)]


@pytest.mark.parametrize("beam,disable_pq,use_scales,L", GRID)
def test_grouped_request_path_equals_the_collapse_of_the_oracles_visited_list(big, mse, orc, beam, disable_pq, use_scales, L):
    """beamwidth {1, 4, 8} x {ADC, exact} x {scales, none} x L {12, 200, 1024}; the grouping, the kind of graph (with / without a has_url
    array) and the entry rule (start nodes given / by the entry table) rotate through the grid so that each meets every parameter value.
    The answer is the collapse of the oracle's disk_greedy_search visited list, the counters are the oracle's."""
    ix = big
    case = GRID.index((beam, disable_pq, use_scales, L))
    name = GROUPINGS[case % len(GROUPINGS)]
    with_url = bool((case // len(GROUPINGS) + case) % 2)
    by_table = bool((case // 3 + case // 12) % 2)
    scales = SCALES if use_scales else None
    nq = 6 if L == 1024 else ix.nq
    starts = ix.by_table if by_table else ix.starts
    url = ix.has_url if with_url else None
    oracle = [ix.oracle(orc, i, L, beam, disable_pq, scales, url, start=starts[i]) for i in range(nq)]
    lists = [(o[1], o[2]) for o in oracle]
    group_of = fit_grouping(name, ix.groupings[name], lists)
    check_conditions(name, group_of, lists)                              # on the oracle's numbers, before the library is called
    groups = mse.RowGroups(group_of)
    ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.qh[:nq], K, None if by_table else starts[:nq],
                                      ix.luts[:nq], scales, disable_pq, beam, L, groups=groups)
    short = 0
    for i in range(nq):
        wi, ws = grouped_cut(oracle[i][1], oracle[i][2], group_of, K)
        assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (name, i)
        assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (oracle[i][3], oracle[i][4], len(oracle[i][1])), (name, i)
        short += int((wi == ID_NONE).any())
    print(f"grouping {name}, has_url array {with_url}, entry table {by_table}: {short} of {nq} queries short")


def test_all_none_grouping_is_the_ungrouped_call_bit_for_bit(big, mse):
    ix = big
    none = mse.RowGroups(ix.groupings["none"])
    for with_url, disable_pq, beam, L, starts in ((True, False, 4, 100, ix.starts), (False, True, 8, 300, None), (True, True, 1, 12, ix.starts)):
        args = (ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.qh, K, starts, ix.luts, SCALES, disable_pq, beam, L)
        a = mse.disk_query_topk(*args)
        b = mse.disk_query_topk(*args, groups=none)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(a[2][c], b[2][c]) for c in COUNTERS)
        assert np.any(a[0] != ID_NONE)


def duplicated_index(ix, mse):
    """ix with a tenth of the rows overwritten by their first neighbour's vector: near-duplicates that a search visits together"""
    rng = np.random.default_rng(41)
    base = ix.base.copy()
    dst = rng.choice(N, N // 10, replace=False)
    base[dst] = ix.base[ix.adj[dst, 0]]
    local = Index.__new__(Index)
    local.__dict__.update(ix.__dict__)
    local.base = base
    local.vecs = mse.VectorList.from_f16s(base, ix.d)
    local.searcher = mse.Searcher(local.vecs)
    return local


def test_deduplication_first_then_the_group_step(big, mse, orc):
    """mse_graph_set_dedup at 0.95: orc.dedup_keep in visit order, then the collapse; both steps remove records."""
    ix = duplicated_index(big, mse)
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    mse.set_dedup(g, 0.95)
    group_of = ix.groupings["runs8"].copy()
    L, beam = 64, 4
    dedup_removed = group_removed = 0
    for disable_pq, scales in ((False, SCALES), (True, None)):
        want = []
        for i in range(ix.nq):
            _, vi, vs, cm, pc = ix.oracle(orc, i, L, beam, disable_pq, scales, ix.has_url)
            keep = orc.dedup_keep(ix.base[vi], 0.95).astype(bool)
            want.append((vi[keep], vs[keep], cm, pc, len(vi)))
            dedup_removed += int((~keep).sum())
        lists = [(w[0], w[1]) for w in want]
        group_of = fit_grouping("runs8", group_of, lists)
        check_conditions("half-none", group_of, lists)                   # (only: some grouped answer differs)
        group_removed += sum(len(w[0]) - int((group_step(w[0], w[1], len(w[0]), group_of)[0] != ID_NONE).sum()) for w in want)
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, scales, disable_pq, beam, L,
                                          groups=mse.RowGroups(group_of))
        for i in range(ix.nq):
            wi, ws = grouped_cut(want[i][0], want[i][1], group_of, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (disable_pq, i)
            assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == want[i][2:], i
    assert dedup_removed > 0 and group_removed > 0


def test_f32_queries_and_device_resident_f16_queries(big, mse, orc):
    ix = big
    L, beam = 64, 4
    g = ix.graphs[True]
    # f32 queries: the RNE f16 copy scores, the tables come from the f32 query
    q32 = (ix.qs * np.float32(1.3)).astype(np.float32)
    q16 = orc.f16_bits(q32)
    oracle = [ix.oracle(orc, i, L, beam, False, SCALES, ix.has_url, qh=q16[i], lut=ix.opq.preprocess_query(q32[i])) for i in range(ix.nq)]
    lists = [(o[1], o[2]) for o in oracle]
    group_of = fit_grouping("half-none", ix.groupings["half-none"], lists)
    check_conditions("half-none", group_of, lists)
    groups = mse.RowGroups(group_of)
    ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, q32, K, ix.starts, None, SCALES, False, beam, L, groups=groups)
    for i in range(ix.nq):
        wi, ws = grouped_cut(oracle[i][1], oracle[i][2], group_of, K)
        assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), i
        assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (oracle[i][3], oracle[i][4], len(oracle[i][1]))
    one = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, q32[3:4], K, ix.starts[3:4], None, SCALES, False, beam, L, groups=groups)
    assert np.array_equal(one[0][0], ids[3]) and np.array_equal(one[1][0], sc[3])            # (one query: through the coalescer)
    # f16 queries that never left the device, in the (pointer, nq) form
    host = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, ix.qh, K, ix.starts, ix.luts, SCALES, False, beam, L, groups=groups)
    oracle = [ix.oracle(orc, i, L, beam, False, SCALES, ix.has_url) for i in range(ix.nq)]
    for i in range(ix.nq):
        wi, ws = grouped_cut(oracle[i][1], oracle[i][2], group_of, K)
        assert np.array_equal(host[0][i], wi) and np.array_equal(host[1][i], ws), i
    qdev = mse.VectorList.from_f16s(ix.qh, ix.d)
    dev = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, g, (qdev.device_ptr, ix.nq), K, ix.starts, ix.luts, SCALES, False, beam, L, groups=groups)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]) and all(np.array_equal(dev[2][c], host[2][c]) for c in COUNTERS)


def test_graph_regime_groups_the_filtered_visited_list(big, mse, orc):
    """A group whose best row is disallowed is represented by its best allowed visited row: the oracle over has_url AND allowed, collapsed."""
    ix = big
    L, beam = 100, 4
    for with_url, fname in ((True, "half"), (False, "short")):
        url = ix.eff_url(fname, with_url)
        oracle = [ix.oracle(orc, i, L, beam, False, SCALES, url) for i in range(ix.nq)]
        lists = [(o[1], o[2]) for o in oracle]
        group_of = fit_grouping("runs8", ix.groupings["runs8"], lists)
        check_conditions("runs8", group_of, lists)
        ids, sc, st = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, ix.graphs[with_url], ix.qh, K, ix.starts, ix.luts, SCALES, False, beam, L,
                                          filter=ix.filters[fname], regime="graph", groups=mse.RowGroups(group_of))
        for i in range(ix.nq):
            wi, ws = grouped_cut(oracle[i][1], oracle[i][2], group_of, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (fname, i)
            assert (int(st["cmps"][i]), int(st["pq_cmps"][i]), int(st["n_visited"][i])) == (oracle[i][3], oracle[i][4], len(oracle[i][1]))
            assert np.all(url[wi[wi != ID_NONE]] == 1)


def test_list_regime_is_the_grouped_exact_answer_over_the_eligible_rows(big, mse, orc):
    """LIST: grouped_topk over {allowed AND has_url} with the bias added, with and without a has_url array, nq of 1, 8, 9 and 20; one group
    of several thousand rows whose best row the filter disallows; a grouping shorter than the graph; LIST with the de-duplication on
    is still refused and writes nothing."""
    ix = big
    rng = np.random.default_rng(19)
    q20 = orc.f16_bits(clustered_rows(orc, 20, ix.d, n_centres=48, seed=79))
    raw = np.stack([orc.score_all(ix.base, q) for q in q20])
    group_of = ix.groupings["cluster"].copy()
    group_of[rng.choice(N, 5000, replace=False)] = 47                    # one group of several thousand rows
    mask = rng.random(N) < 0.3
    members = np.flatnonzero(group_of == 47)
    assert members.size > 4000
    mask[members[np.argmax(raw[0][members])]] = False                     # ... whose best row (for the first query) is disallowed
    mask[members[:2000]] = True
    flt = mse.RowFilter(mask)
    for gname, gr in (("cluster", group_of), ("short", ix.groupings["short"])):
        groups = mse.RowGroups(gr)
        for with_url in (True, False):
            eligible = mask & (ix.has_url != 0) if with_url else mask
            for scales in (None, SCALES):
                score = raw.copy()
                if scales is not None:
                    rows = np.flatnonzero(eligible)
                    with np.errstate(over="ignore"):
                        bias = np.array([orc.descriptor_product(scales, ix.desc, int(r)) for r in rows], np.int64)
                    score[:, rows] += bias
                for nq in (1, 8, 9, 20):
                    ids, sc, st = mse.disk_query_topk(ix.searcher, None, ix.gcodes, ix.graphs[with_url], q20[:nq], K, None, None, scales, True, 4, 50,
                                                      filter=flt, regime="list", groups=groups)
                    for i in range(nq):
                        ws, wi = grouped_topk(score[i], gr, K, allowed=eligible)
                        assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (gname, with_url, nq, i)
                    assert np.all(st["n_visited"] == eligible.sum()) and np.all(st["cmps"] == eligible.sum()) and np.all(st["pq_cmps"] == 0)
                # the grouping changes the answer: the ungrouped LIST call differs for some query
                plain = mse.disk_query_topk(ix.searcher, None, ix.gcodes, ix.graphs[with_url], q20[:8], K, None, None, scales, True, 4, 50,
                                            filter=flt, regime="list")
                assert gname == "short" or not np.array_equal(plain[0], ids[:8])
    g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
    mse.set_dedup(g, 0.95)
    with pytest.raises(mse.MseError, match="de-duplicate"):
        mse.disk_query_topk(ix.searcher, None, ix.gcodes, g, q20[:2], K, None, None, None, True, 4, 50, filter=flt, regime="list",
                            groups=mse.RowGroups(group_of))


def test_auto_is_the_explicit_call_at_the_plans_answer(big, mse):
    ix = big
    rng = np.random.default_rng(3)
    rows = rng.choice(N, 3907, replace=False)
    groups = mse.RowGroups(ix.groupings["cluster"])
    args = (ix.searcher, ix.gpq, ix.gcodes, ix.graphs[True], ix.qh, K, ix.starts, ix.luts, SCALES, False, 4, 200)
    for count, want in ((3907, ("graph", 1024)), (3906, ("list", 200))):
        flt = mse.RowFilter(rows[:count], n_rows=N)
        assert mse.filtered_plan(N, flt.count, 200) == want
        auto = mse.disk_query_topk(*args, filter=flt, groups=groups)
        explicit = mse.disk_query_topk(*args[:-1], want[1], filter=flt, regime=want[0], groups=groups)
        ungrouped = mse.disk_query_topk(*args, filter=flt)
        assert np.array_equal(auto[0], explicit[0]) and np.array_equal(auto[1], explicit[1])
        assert all(np.array_equal(auto[2][c], explicit[2][c]) and np.array_equal(auto[2][c], ungrouped[2][c]) for c in COUNTERS)
        assert np.any(auto[0] != ID_NONE) and not np.array_equal(auto[0], ungrouped[0])


def test_one_query_calls_and_tickets_share_submissions_by_grouping(big, mse, orc):
    """One-query calls from threads, and tickets from one thread, in flight together for grouping A, grouping B, no grouping, and
    grouping A with a filter: every caller gets the row of its own batch call, and the coalescer shows shared submissions."""
    ix = big
    g = ix.graphs[True]
    T, L, beam = 48, 48, 4
    qs = clustered_rows(orc, T, ix.d, n_centres=48, seed=501).astype(np.float32)
    a, b = mse.RowGroups(ix.groupings["cluster"]), mse.RowGroups(ix.groupings["runs8"])
    kinds = [dict(groups=a), dict(groups=b), dict(), dict(groups=a, filter=ix.filters["half"], regime="graph")]
    lone = mse.Searcher(ix.vecs)
    want = [None] * T
    for kd in range(len(kinds)):                                          # the batch call of every kind: 12 queries each
        rows = list(range(kd, T, len(kinds)))
        batch = mse.disk_query_topk(lone, None, ix.gcodes, g, qs[rows], K, None, None, SCALES, True, beam, L, **kinds[kd])
        for j, i in enumerate(rows):
            want[i] = (batch[0][j], batch[1][j], {c: batch[2][c][j] for c in COUNTERS})
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
        assert np.array_equal(got[i][0][0], want[i][0]) and np.array_equal(got[i][1][0], want[i][1]), i
        assert all(got[i][2][c][0] == want[i][2][c] for c in COUNTERS), i
    after = mse.coalescer_stats(g)
    assert after["requests"] - before["requests"] == 3 * T
    assert after["max_pass_queries"] > 1 and after["passes"] - before["passes"] < 3 * T       # requests shared submissions
    tickets = [mse.QueryTickets(ix.searcher, None, ix.gcodes, g, K, True, beam, L, **kd) for kd in kinds]
    before = mse.coalescer_stats(g)
    for i in range(T):
        tickets[i % len(kinds)].submit(qs[i], SCALES, key=i)
    done = {}
    while len(done) < T:
        back = tickets[0].collect(timeout_us=5_000_000)
        assert back, "no ticket came back within five seconds"
        for key, ids, sc in back:
            done[key] = (ids, sc)
    for i in range(T):
        assert np.array_equal(done[i][0][0], want[i][0]) and np.array_equal(done[i][1][0], want[i][1]), i
    after = mse.coalescer_stats(g)
    assert after["requests"] - before["requests"] == T and after["passes"] - before["passes"] < T


def test_one_handle_across_calls_equals_fresh_handles(big, mse, orc):
    """On one searcher: the group step in its global-table form (the hook at cap 8448), a small grouped request, an ungrouped request,
    a grouped request under another grouping -- each equals the same call on a fresh searcher."""
    ix = big
    rng = np.random.default_rng(23)
    hook_g = make_grouping("random", rng)
    ids, sc = make_lists(8448, [8448, 4097], hook_g, rng)
    hook_groups = mse.RowGroups(hook_g)
    a, b = mse.RowGroups(ix.groupings["cluster"]), mse.RowGroups(ix.groupings["cluster"] // 2)
    req = (None, ix.gcodes, ix.graphs[True], ix.qh, K, ix.starts, None, SCALES, True, 4, 64)
    calls = [lambda s: run_hook(mse, s, hook_groups, ids, sc, [8448, 4097]),
             lambda s: mse.disk_query_topk(s, *req, groups=a)[:2],
             lambda s: mse.disk_query_topk(s, *req)[:2],
             lambda s: mse.disk_query_topk(s, *req, groups=b)[:2]]
    one = mse.Searcher(ix.vecs)
    seq = [call(one) for call in calls]
    for j, call in enumerate(calls):
        fresh = call(mse.Searcher(ix.vecs))
        assert np.array_equal(seq[j][0], fresh[0]) and np.array_equal(seq[j][1], fresh[1]), j
    assert not np.array_equal(seq[1][0], seq[2][0]) and not np.array_equal(seq[3][0], seq[2][0]) and not np.array_equal(seq[1][0], seq[3][0])


def test_grouped_argument_errors_write_nothing(big, mse):
    """null grouping, a grouping longer than the graph, k = 0, a bad regime together with a filter: non-zero, a message, outputs
    untouched -- in every entry point; the call's own checks come before the grouping's."""
    from mse import ffi
    ix = big
    L = ffi.lib()
    g = ix.graphs[False]
    too_long = mse.RowGroups(np.zeros(N + 1, np.uint32))
    ok = mse.RowGroups(ix.groupings["runs8"])
    flt = ix.filters["half"]
    q16 = np.ascontiguousarray(ix.qh[:2])
    q32 = np.ascontiguousarray(ix.qs[:2], np.float32)
    st = np.ascontiguousarray(ix.starts[:2])
    cases = [(None, None, 1, K, "null grouping"), (too_long._h, None, 1, K, "longer"), (ok._h, None, 1, 0, "bad k"),
             (ok._h, flt._h, 7, K, "regime"), (None, flt._h, 7, K, "regime"), (None, None, 1, 0, "bad k"), (None, flt._h, 1, K, "null grouping")]
    for grp, f, regime, k, word in cases:
        oi, os_, nv = np.full((2, K), 123, np.uint32), np.full((2, K), 456, np.int64), np.full(2, 789, np.uint32)
        outs = (oi.ctypes.data_as(ffi.u32p), os_.ctypes.data_as(ffi.i64p), nv.ctypes.data_as(ffi.u32p), None, None)
        untouched = lambda: np.all(oi == 123) and np.all(os_ == 456) and np.all(nv == 789)   # noqa: E731
        assert L.mse_disk_query_topk_grouped(ix.searcher._h, None, None, g._h, grp, f, regime, st.ctypes.data_as(ffi.u32p), q16.ctypes.data_as(ffi.u16p),
                                             None, None, 2, 1, 4, 50, k, *outs) != 0
        assert word in ffi.last_error() and untouched(), (word, ffi.last_error())
        assert L.mse_disk_query_topk_grouped_f32(ix.searcher._h, None, None, g._h, grp, f, regime, st.ctypes.data_as(ffi.u32p),
                                                 q32.ctypes.data_as(ffi.f32p), None, 2, 1, 4, 50, k, *outs) != 0
        assert word in ffi.last_error() and untouched(), (word, ffi.last_error())
        t = C.c_void_p()
        assert L.mse_disk_query_submit_grouped_f32(ix.searcher._h, None, None, g._h, grp, f, regime, q32.ctypes.data_as(ffi.f32p), None, 2, 1, 4, 50, k,
                                                   *outs, None, None, C.byref(t)) != 0
        assert word in ffi.last_error() and untouched() and not t.value, (word, ffi.last_error())
    with pytest.raises(mse.MseError, match="longer"):
        mse.disk_query_topk(ix.searcher, None, None, g, ix.qh[:2], K, ix.starts[:2], None, None, True, 4, 50, groups=too_long)
