"""Grouped search (include/mse.h mse_groups): one result per group -- the best eligible row of each group in the search's own total
order -- equals the numpy collapse of the oracle's full ranking, bit for bit, on the prefix path, the widened prefix and the dense path,
with and without a filter, for the f16 brute force and the flat index; and the collapse kernel alone against a numpy walk."""

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY
from grouped_ref import GROUP_NONE, I64_MIN, ID_NONE, collapse_positions, grouped_topk

pytestmark = pytest.mark.gpu
D = 1152
MODES = {"exact": 1, "mfma": 2, "auto": 0}
F32_LOWEST = -np.finfo(np.float32).max

_scores = {}   # (n, nq) -> the oracle's scores [nq][n] of the first nq queries against the first n rows: computed once, never written


def oracle_scores(orc, n, nq):
    if (n, nq) not in _scores:
        base = orc.gen_rows_f16(SEED_BASE, 0, n)
        q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
        sc = np.stack([orc.score_all(base, q[i]) for i in range(nq)])
        sc.setflags(write=False)
        _scores[(n, nq)] = sc
    return _scores[(n, nq)]


def reference(scores, group_of, k, allowed=None):
    out = [grouped_topk(scores[i], group_of, k, allowed) for i in range(scores.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def make_groups(kind, n, rng):
    if kind == "none":
        return np.full(n, GROUP_NONE, np.uint32)
    if kind == "random3":
        g = rng.integers(0, max(n // 3, 1), n).astype(np.uint32)
        g[rng.random(n) < 0.2] = GROUP_NONE
        return g
    assert kind == "runs8"
    return (np.arange(n, dtype=np.uint32) // 8) * 8   # the row id of the run's first member


def searcher_of(mse, orc, n):
    return mse.Searcher(mse.VectorList.from_f16s(orc.gen_rows_f16(SEED_BASE, 0, n), D))


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
@pytest.mark.parametrize("n,nq,k", [(1, 1, 1), (5000, 1, 1000), (20000, 9, 10), (20000, 130, 10), (21011, 320, 10), (7000, 700, 5)])
def test_grouped_matches_collapsed_oracle(gpu, mse, orc, mode, n, nq, k):
    rng = np.random.default_rng(n * 31 + nq)
    scores = oracle_scores(orc, n, nq)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    s = searcher_of(mse, orc, n)
    mask = rng.random(n) < 0.5
    if not mask.any():
        mask[0] = True
    for kind in ("none", "random3", "runs8"):
        group_of = make_groups(kind, n, rng)
        g = mse.RowGroups(group_of)
        assert len(g) == n
        assert g.count == int((group_of == GROUP_NONE).sum()) + np.unique(group_of[group_of != GROUP_NONE]).size
        for allow in (None, mask):
            sc, ids = s.bruteforce_topk(q, k, MODES[mode], allow=allow, groups=g)
            ws, wi = reference(scores, group_of, k, allow)
            assert np.array_equal(ids, wi) and np.array_equal(sc, ws), (kind, allow is not None)
            if kind == "none":   # every row a group of its own: exactly the ungrouped answer
                us, ui = s.bruteforce_topk(q, k, MODES[mode], allow=allow)
                assert np.array_equal(ids, ui) and np.array_equal(sc, us), (kind, allow is not None)
                if mode == "mfma":
                    assert s.grouped_stats()[2] == 0
        g.close()


@pytest.mark.parametrize("nq", [9, 130])
def test_dense_path_large_k(gpu, mse, orc, nq):
    # one group holds a random 60 % of the rows: the best 1984 rows of a query hold about 0.4 x 1984 + 1 = 795 (+- 18) groups, fewer than
    # k = 1000, so no prefix the selection can return is long enough
    n, k = 6000, 1000
    rng = np.random.default_rng(nq)
    scores = oracle_scores(orc, n, nq)
    group_of = np.where(rng.random(n) < 0.6, 17, GROUP_NONE).astype(np.uint32)
    for i in range(nq):
        order = np.lexsort((np.arange(n), -scores[i]))[:1984]
        assert collapse_positions(order, group_of).size < k
    s = searcher_of(mse, orc, n)
    sc, ids = s.bruteforce_topk(orc.gen_rows_f16(SEED_QUERY, 0, nq), k, mse.MODE_MFMA, groups=group_of)
    ws, wi = reference(scores, group_of, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert s.grouped_stats() == (0, 0, nq)


@pytest.mark.parametrize("nq,mode", [(1, "exact"), (40, "mfma")])
def test_dense_path_short_answer(gpu, mse, orc, nq, mode):
    # every row but five in one group: six results, four empty slots -- and no other member of the group in them
    n, k = 4000, 10
    rng = np.random.default_rng(5)
    scores = oracle_scores(orc, n, 40)[:nq]
    group_of = np.full(n, 3, np.uint32)
    loners = rng.choice(n, 5, replace=False)
    group_of[loners] = GROUP_NONE
    s = searcher_of(mse, orc, n)
    sc, ids = s.bruteforce_topk(orc.gen_rows_f16(SEED_QUERY, 0, nq), k, MODES[mode], groups=group_of)
    ws, wi = reference(scores, group_of, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert (ids[:, 6:] == ID_NONE).all() and (sc[:, 6:] == I64_MIN).all() and (ids[:, :6] != ID_NONE).all()
    assert (np.isin(ids[:, :6], loners).sum(axis=1) == 5).all()   # the five loners and ONE member of the group
    assert s.grouped_stats()[2] == nq


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_ties_lower_id_represents(gpu, mse, orc, mode):
    n, nq, k = 3000, 12, 8
    base = orc.gen_rows_f16(SEED_BASE, 0, n).copy()
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq).copy()
    q[:, :] = base[7]                       # row 7 is every query's best match ...
    base[[7, 100, 640, 2047, 2999]] = base[7]   # ... and so are its copies
    group_of = np.full(n, GROUP_NONE, np.uint32)
    group_of[[100, 640]] = 5                # a duplicate inside one group: the lower id represents it
    group_of[[7, 2999]] = 9                 # ... and in another; 2047 is on its own.  Equal scores across groups: ascending id
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = s.bruteforce_topk(q, k, MODES[mode], groups=group_of)
    scores = np.stack([orc.score_all(base, q[i]) for i in range(nq)])
    ws, wi = reference(scores, group_of, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert list(ids[0, :3]) == [7, 100, 2047] and sc[0, 0] == sc[0, 1] == sc[0, 2]
    assert 640 not in ids[0] and 2999 not in ids[0]


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_filter_interplay(gpu, mse, orc, mode):
    n, nq, k = 5000, 10, 20
    rng = np.random.default_rng(77)
    scores = oracle_scores(orc, n, nq)
    group_of = rng.integers(0, 200, n).astype(np.uint32)
    best = np.array([[np.flatnonzero(group_of == g)[np.lexsort((np.flatnonzero(group_of == g), -scores[i][group_of == g]))[0]] for g in range(200)]
                     for i in range(nq)])
    mask = np.ones(n, bool)
    mask[best[0]] = False                   # the best row of every group (for query 0) is disallowed
    mask[group_of == 11] = False            # group 11 has no allowed row at all
    s = searcher_of(mse, orc, n)
    sc, ids = s.bruteforce_topk(orc.gen_rows_f16(SEED_QUERY, 0, nq), k, MODES[mode], allow=mask, groups=group_of)
    ws, wi = reference(scores, group_of, k, mask)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert mask[ids].all() and not (group_of[ids] == 11).any()
    assert not np.isin(ids[0], best[0]).any()
    for j in range(k):   # each result of query 0 is the best ALLOWED row of its group
        members = np.flatnonzero((group_of == group_of[ids[0, j]]) & mask)
        assert ids[0, j] == members[np.lexsort((members, -scores[0][members]))[0]]


def test_short_grouping_offset_and_k_above_count(gpu, mse, orc):
    import torch
    n, nq = 3000, 9
    scores = oracle_scores(orc, n, nq)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    s = searcher_of(mse, orc, n)
    # a grouping shorter than the base: rows at and past its length are groups of their own
    short = (np.arange(1000, dtype=np.uint32) // 50) * 50
    for mode in MODES.values():
        sc, ids = s.bruteforce_topk(q, 40, mode, groups=short)
        ws, wi = reference(scores, short, 40)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    # the device form with an id offset: groups by local id, the offset on the way out only
    group_of = np.random.default_rng(3).integers(0, 300, n).astype(np.uint32)
    g = mse.RowGroups(group_of)
    qd = torch.from_numpy(q.view(np.int16).copy()).cuda()
    out_s = torch.zeros((nq, 10), dtype=torch.int64, device="cuda")
    out_i = torch.zeros((nq, 10), dtype=torch.int32, device="cuda")
    off = 1 << 20
    ws, wi = reference(scores, group_of, 10)
    for mode in MODES.values():
        torch.cuda.synchronize()
        s.bruteforce_topk_dev(qd.data_ptr(), nq, 10, out_s.data_ptr(), out_i.data_ptr(), mode, id_offset=off, groups=g)
        mse.ffi.check(mse.ffi.lib().mse_device_synchronize())
        assert np.array_equal(out_i.cpu().numpy().view(np.uint32), wi + off) and np.array_equal(out_s.cpu().numpy(), ws)
    # a grouping made from device memory is the same grouping
    gd = mse.RowGroups.from_device(torch.from_numpy(group_of.view(np.int32).copy()).cuda().data_ptr(), n)
    assert len(gd) == n and gd.count == g.count == np.unique(group_of).size
    sc, ids = s.bruteforce_topk(q, 10, mse.MODE_MFMA, groups=gd)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    # k above the number of groups: count results, then padding
    few = mse.RowGroups((np.arange(n, dtype=np.uint32) % 7))
    assert few.count == 7
    for mode in MODES.values():
        sc, ids = s.bruteforce_topk(q, 12, mode, groups=few)
        ws7, wi7 = reference(scores, np.arange(n, dtype=np.uint32) % 7, 12)
        assert np.array_equal(ids, wi7) and np.array_equal(sc, ws7)
        assert (ids[:, 7:] == ID_NONE).all() and (ids[:, :7] != ID_NONE).all()


# ---- the collapse kernel alone ------------------------------------------------------------------------------------------------------------
def collapse_on_device(mse, s, g, ids, k):
    from mse import ffi
    ids = np.ascontiguousarray(ids, np.uint32)
    nq, n_list = ids.shape
    kept = np.full((nq, k), 7, np.uint32)
    reps = np.full(nq, 7, np.uint32)
    ffi.check(ffi.lib().mse_debug_collapse_topk(s._h, g._h, ids.ctypes.data_as(ffi.u32p), n_list, nq, k, kept.ctypes.data_as(ffi.u32p),
                                                reps.ctypes.data_as(ffi.u32p)), "collapse_topk")
    return kept, reps


def check_collapse(mse, s, group_of, ids, k):
    g = mse.RowGroups(group_of)
    kept, reps = collapse_on_device(mse, s, g, ids, k)
    for i in range(ids.shape[0]):
        valid = ids[i][ids[i] != ID_NONE]
        want = collapse_positions(valid, group_of)
        assert reps[i] == want.size, i
        m = min(k, want.size)
        assert np.array_equal(kept[i, :m], want[:m]) and (kept[i, m:] == ID_NONE).all(), i
    g.close()


@pytest.mark.parametrize("n_list", [1, 63, 64, 65, 2048])
def test_collapse_kernel_list_lengths(gpu, mse, orc, n_list):
    rng = np.random.default_rng(n_list)
    n_rows, nq = 5000, 7
    s = searcher_of(mse, orc, 64)
    ids = np.stack([rng.permutation(n_rows)[:n_list] for _ in range(nq)]).astype(np.uint32)
    random3 = make_groups("random3", n_rows, rng)
    for k in (1, min(n_list, 10), n_list):
        check_collapse(mse, s, random3, ids, k)
    check_collapse(mse, s, np.full(n_rows, 42, np.uint32), ids, 5)                     # all entries in one group
    check_collapse(mse, s, np.full(n_rows, GROUP_NONE, np.uint32), ids, n_list)        # all NONE
    check_collapse(mse, s, np.arange(n_rows, dtype=np.uint32)[::-1].copy(), ids, n_list)   # as many distinct groups as entries
    short = np.where(random3[:100] < 100, random3[:100], GROUP_NONE).astype(np.uint32)
    check_collapse(mse, s, short, ids, n_list)                                         # entries past a short grouping
    # tail padding: the last third of every list is empty
    padded = ids.copy()
    padded[:, n_list - n_list // 3:] = ID_NONE
    check_collapse(mse, s, random3, padded, max(n_list // 2, 1))
    if n_list > 2:
        padded[0, :] = ID_NONE   # ... and an empty list
        check_collapse(mse, s, random3, padded, 3)


def test_collapse_kernel_colliding_groups(gpu, mse, orc):
    # group ids that are equal modulo every power of two up to 8192, and group ids that share one slot of the kernel's own table
    # (the top 12 bits of id x 2654435761 mod 2^32): the probe sequence must keep them apart and in order
    rng = np.random.default_rng(8)
    n_rows, n_list, nq = 1 << 21, 2048, 4
    s = searcher_of(mse, orc, 64)
    modulo = (5 + 8192 * np.arange(250)).astype(np.uint32)
    all_ids = np.arange(n_rows, dtype=np.uint64)
    slot = ((all_ids * 2654435761) & 0xFFFFFFFF) >> 20
    same_slot = np.flatnonzero(slot == slot[12345])[:250].astype(np.uint32)
    assert same_slot.size >= 200
    for pool in (modulo, same_slot, np.concatenate([modulo, same_slot])):
        group_of = np.full(n_rows, GROUP_NONE, np.uint32)
        rows = rng.choice(n_rows, 4 * n_list, replace=False)
        group_of[rows] = rng.choice(pool, rows.size)
        ids = np.stack([rng.permutation(rows)[:n_list] for _ in range(nq)]).astype(np.uint32)
        check_collapse(mse, s, group_of, ids, n_list)
        check_collapse(mse, s, group_of, ids, 100)


def test_errors_write_nothing(gpu, mse, orc):
    from mse import ffi
    lib = ffi.lib()
    n, nq = 2000, 3
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = np.ascontiguousarray(orc.gen_rows_f16(SEED_QUERY, 0, nq))
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    # an id at or past n_rows: an error at creation, nothing is made
    bad = np.array([0, 1, 5, 4], np.uint32)
    assert not lib.mse_groups_from_host(bad.ctypes.data_as(ffi.u32p), 4)
    assert b"not below n_rows" in lib.mse_last_error()
    with pytest.raises(mse.MseError):
        mse.RowGroups(bad)
    ok = mse.RowGroups(np.array([0, 3, GROUP_NONE, 3], np.uint32))
    assert len(ok) == 4 and ok.count == 3
    g = mse.RowGroups(np.zeros(n, np.uint32))
    longer = mse.RowGroups(np.zeros(n + 1, np.uint32))
    sc = np.full((nq, 10), 7, np.int64)
    ids = np.full((nq, 10), 7, np.uint32)
    qp, sp, ip = q.ctypes.data_as(ffi.u16p), sc.ctypes.data_as(ffi.i64p), ids.ctypes.data_as(ffi.u32p)
    for mode in (0, 1, 2):
        assert lib.mse_bruteforce_topk_grouped_f16(s._h, longer._h, None, qp, nq, 10, mode, sp, ip) == -1
        assert b"longer than the base" in lib.mse_last_error()
        assert lib.mse_bruteforce_topk_grouped_f16(s._h, None, None, qp, nq, 10, mode, sp, ip) == -1
        assert b"null grouping" in lib.mse_last_error()
        assert lib.mse_bruteforce_topk_grouped_f16(s._h, g._h, None, qp, nq, 1985, mode, sp, ip) == -1
        assert b"k too large" in lib.mse_last_error()
    assert lib.mse_bruteforce_topk_grouped_f16(s._h, g._h, None, qp, nq, 10, 9, sp, ip) == -1
    assert b"unknown mode" in lib.mse_last_error()
    assert lib.mse_bruteforce_topk_grouped_f16_dev(s._h, None, None, None, nq, 10, 0, 0, None, None) == -1
    assert b"null grouping" in lib.mse_last_error()
    assert (sc == 7).all() and (ids == 7).all()
    idx = mse.ScalarQuantizerIndex(D)
    idx.add(orc.f16_to_f32(base))
    dist = np.full((1, 10), 7, np.float32)
    lab = np.full((1, 10), 7, np.int64)
    qf = np.ascontiguousarray(orc.f16_to_f32(q[:1]))
    args = (qf.ctypes.data_as(ffi.f32p), 1, 10, dist.ctypes.data_as(ffi.f32p), lab.ctypes.data_as(ffi.i64p))
    assert lib.mse_index_search_grouped(idx._h, None, None, *args) == -1
    assert b"null grouping" in lib.mse_last_error()
    assert lib.mse_index_search_grouped(idx._h, longer._h, None, *args) == -1
    assert b"longer than the base" in lib.mse_last_error()
    assert (dist == 7).all() and (lab == 7).all()
    idx.close()


def test_handle_reuse(gpu, mse, orc):
    # one Searcher: a dense-path grouped call, an ungrouped call, a filtered call, a grouped call on the prefix path -- each equals the
    # oracle and a fresh handle
    n, nq, k = 6000, 20, 10
    rng = np.random.default_rng(12)
    scores = oracle_scores(orc, n, 130)[:nq]
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    big = np.where(rng.random(n) < 0.9995, 1, GROUP_NONE).astype(np.uint32)   # about three rows outside one huge group: the dense path
    runs = make_groups("runs8", n, rng)
    mask = rng.random(n) < 0.5
    none = np.full(n, GROUP_NONE, np.uint32)
    vl = mse.VectorList.from_f16s(base, D)
    s = mse.Searcher(vl)
    calls = [dict(groups=big), dict(), dict(allow=mask), dict(groups=runs), dict(groups=big, allow=mask)]
    for kw in calls:
        sc, ids = s.bruteforce_topk(q, k, mse.MODE_MFMA, **kw)
        ws, wi = reference(scores, kw.get("groups", none), k, kw.get("allow"))
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), sorted(kw)
        if "groups" in kw:
            assert (s.grouped_stats()[2] == nq) == (kw["groups"] is big), sorted(kw)
        fresh = mse.Searcher(vl)
        fs, fi = fresh.bruteforce_topk(q, k, mse.MODE_MFMA, **kw)
        fresh.close()
        assert np.array_equal(ids, fi) and np.array_equal(sc, fs), sorted(kw)


# ---- flat index ---------------------------------------------------------------------------------------------------------------------------
def index_rows(orc, n, seed):
    rng = np.random.default_rng(seed)
    return orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, n)) * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)


def index_of(mse, rows):
    idx = mse.ScalarQuantizerIndex(D)
    idx.add(rows)
    return idx


def collapse_ranking(res, group_of, k):
    """The index's own ranking (labels best first, -1 padded at the tail) collapsed in numpy, the first k."""
    nq = res.labels.shape[0]
    wd = np.full((nq, k), F32_LOWEST, np.float32)
    wl = np.full((nq, k), -1, np.int64)
    reps = np.zeros(nq, np.int64)
    for i in range(nq):
        valid = res.labels[i] >= 0
        keep = collapse_positions(res.labels[i][valid], group_of)
        reps[i] = keep.size
        keep = keep[:k]
        wd[i, :keep.size] = res.distances[i][valid][keep]
        wl[i, :keep.size] = res.labels[i][valid][keep]
    return wd, wl, reps


def same(res, wd, wl):
    return np.array_equal(res.labels, wl) and np.array_equal(res.distances.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("nq", [3, 40])
def test_flat_index_grouped_equals_collapsed_full_ranking(gpu, mse, orc, nq):
    n, k = 1900, 10
    rng = np.random.default_rng(nq)
    idx = index_of(mse, index_rows(orc, n, nq))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq)) + np.float32(1e-3)
    mask = rng.random(n) < 0.5
    for kind in ("none", "random3", "runs8"):
        group_of = make_groups(kind, n, rng)
        for allow in (None, mask):
            full = idx.search(qf, n, allow=allow)   # k = n: the full ranking
            for kk in (k, 700):
                wd, wl, _ = collapse_ranking(full, group_of, kk)
                assert same(idx.search(qf, kk, allow=allow, groups=group_of), wd, wl), (kind, allow is not None, kk)
    idx.close()


@pytest.mark.parametrize("nq", [3, 40])
def test_flat_index_grouped_prefix(gpu, mse, orc, nq):
    n, k = 12000, 10
    rng = np.random.default_rng(nq + 1)
    idx = index_of(mse, index_rows(orc, n, nq))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq)) + np.float32(1e-3)
    group_of = make_groups("random3", n, rng)
    wd, wl, reps = collapse_ranking(idx.search(qf, 1984), group_of, k)
    assert (reps >= k).all()   # a prefix of the order collapses to a prefix of the collapsed order: the top 1984 decide the first k groups
    assert same(idx.search(qf, k, groups=group_of), wd, wl)
    idx.close()


@pytest.mark.parametrize("nq", [3, 40])
def test_flat_index_grouped_dense_path(gpu, mse, orc, nq):
    # six groups partition all rows but five: eleven results exist, and the eleventh is thousands of rows down the ranking
    n, k = 4000, 10
    rng = np.random.default_rng(nq + 2)
    idx = index_of(mse, index_rows(orc, n, nq))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq)) + np.float32(1e-3)
    group_of = rng.integers(0, 6, n).astype(np.uint32)
    group_of[rng.choice(n, 5, replace=False)] = GROUP_NONE
    parts = [idx.search(qf, 1, allow=(group_of == g)) for g in range(6)] + [idx.search(qf, 5, allow=(group_of == GROUP_NONE))]
    cd = np.concatenate([p.distances for p in parts], axis=1)
    cl = np.concatenate([p.labels for p in parts], axis=1)
    wd, wl = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    for i in range(nq):
        order = np.lexsort((cl[i], -cd[i].astype(np.float64)))[:k]
        wd[i], wl[i] = cd[i][order], cl[i][order]
    assert same(idx.search(qf, k, groups=group_of), wd, wl)
    got = idx.search(qf, 12, groups=group_of)   # more than there are groups: eleven results and one empty slot
    assert (got.labels[:, :11] >= 0).all() and (got.labels[:, 11] == -1).all() and (got.distances[:, 11] == F32_LOWEST).all()
    assert np.array_equal(got.labels[:, :10], wl)
    idx.close()


def test_flat_index_old_grouping_after_add(gpu, mse, orc):
    n0, n1, nq, k = 3000, 500, 20, 10
    x = index_rows(orc, n0 + n1, 4)
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq))
    idx = index_of(mse, x[:n0])
    group_of = make_groups("runs8", n0, None)
    g = mse.RowGroups(group_of)
    idx.add(x[n0:] * 4.0)   # new rows that outscore every old one: groups of their own, so they all appear
    got = idx.search(qf, k, groups=g)
    wd, wl, _ = collapse_ranking(idx.search(qf, 1984), group_of, k)
    assert same(got, wd, wl) and (got.labels >= n0).all()
    idx.close()


def test_flat_index_coalesced_requests_grouped_by_filter_and_grouping(gpu, mse, orc):
    import threading
    n, T, k = 20000, 64, 10
    rng = np.random.default_rng(21)
    idx = index_of(mse, index_rows(orc, n, 5))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, T))
    fa = mse.RowFilter(rng.random(n) < 0.4)
    ga, gb = mse.RowGroups(make_groups("random3", n, rng)), mse.RowGroups(make_groups("runs8", n, rng))
    pairs = [(None, None), (fa, None), (None, ga), (fa, ga), (None, gb)]
    alone = [idx.search(qf[i], k, allow=pairs[i % 5][0], groups=pairs[i % 5][1]) for i in range(T)]
    before = idx.stats()["passes"]
    got = [None] * T
    bar = threading.Barrier(T)

    def body(i):
        bar.wait()
        got[i] = idx.search(qf[i], k, allow=pairs[i % 5][0], groups=pairs[i % 5][1])
    th = [threading.Thread(target=body, args=(i,)) for i in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(T):
        assert same(got[i], alone[i].distances, alone[i].labels), i
    assert idx.stats()["passes"] - before < T
    idx.close()
