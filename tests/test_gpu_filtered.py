"""Filtered brute-force search (include/mse.h mse_filter): top-k over an allowed-row set equals the unfiltered search on a base made
of the allowed rows alone, ids mapped back -- bit for bit, in every mode and on both the masked-scan and the sparse path."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152
MODES = {"exact": 1, "mfma": 2, "auto": 0}
I64_MIN = np.iinfo(np.int64).min
ID_NONE = 0xFFFFFFFF


def subset_oracle(orc, base, mask, q, k):
    """orc.bruteforce_topk over base[mask], ids mapped through flatnonzero(mask)."""
    allowed = np.flatnonzero(mask)
    nq = q.reshape(-1, base.shape[1]).shape[0]
    if allowed.size == 0:
        return np.full((nq, k), I64_MIN, np.int64), np.full((nq, k), ID_NONE, np.uint32)
    ws, wi = orc.bruteforce_topk(base[allowed], q, k)
    ids = np.where(wi == ID_NONE, ID_NONE, allowed[np.minimum(wi, allowed.size - 1)]).astype(np.uint32)
    return ws, ids


def make_mask(kind, n, k, rng):
    m = np.zeros(n, bool)
    if kind == "none":
        pass
    elif kind == "one":
        m[rng.integers(0, n)] = True
    elif kind in ("fewer_than_k", "exactly_k"):
        c = min(n, max(k // 2, 1) if kind == "fewer_than_k" else k)
        m[rng.choice(n, c, replace=False)] = True
    elif kind == "all":
        m[:] = True
    else:
        m = rng.random(n) < {"1%": 0.01, "50%": 0.5, "99%": 0.99}[kind]
    return m


def run(mse, s, q, k, mode, mask):
    return s.bruteforce_topk(q, k, MODES[mode], allow=mask)


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
@pytest.mark.parametrize("density", ["1%", "50%"])
@pytest.mark.parametrize("n,nq,k", [(1, 1, 1), (5000, 1, 1000), (20000, 9, 10), (20000, 130, 10), (15000, 192, 10), (30000, 256, 10),
                                    (21011, 320, 10), (7000, 700, 5), (40000, 9, 1000)])
def test_filtered_matches_subset_oracle(gpu, mse, orc, mode, density, n, nq, k):
    rng = np.random.default_rng(n * 31 + nq)
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    mask = make_mask(density, n, k, rng)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = run(mse, s, q, k, mode, mask)
    ws, wi = subset_oracle(orc, base, mask, q, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
@pytest.mark.parametrize("density", ["none", "one", "fewer_than_k", "exactly_k", "1%", "50%", "99%", "all"])
@pytest.mark.parametrize("n,nq,k", [(3000, 130, 10), (2000, 9, 100)])
def test_filter_densities(gpu, mse, orc, mode, density, n, nq, k):
    rng = np.random.default_rng(len(density) * 7 + n)
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    mask = make_mask(density, n, k, rng)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    f = mse.RowFilter(mask)
    assert len(f) == n and f.count == int(mask.sum())
    sc, ids = run(mse, s, q, k, mode, f)
    ws, wi = subset_oracle(orc, base, mask, q, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)


@pytest.mark.parametrize("d,nq", [(192, 300), (448, 290), (128, 320)])
def test_filtered_other_widths(gpu, mse, orc, d, nq):
    # other ring depths of the scan (d / 64 = 3, 7, 2 K blocks)
    rng = np.random.default_rng(d)
    base = orc.gen_rows_f16(SEED_BASE, 0, 6000, d)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq, d)
    mask = rng.random(6000) < 0.3
    s = mse.Searcher(mse.VectorList.from_f16s(base, d))
    ws, wi = subset_oracle(orc, base, mask, q, 6)
    for mode in MODES:
        sc, ids = run(mse, s, q, 6, mode, mask)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), mode


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
def test_all_allowed_equals_unfiltered(gpu, mse, orc, mode):
    n, nq, k = 20000, 256, 10
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    us, ui = s.bruteforce_topk(q, k, MODES[mode])
    fs, fi = run(mse, s, q, k, mode, np.ones(n, bool))
    assert np.array_equal(ui, fi) and np.array_equal(us, fs)


@pytest.mark.parametrize("nq", [128, 192, 256, 320])
def test_epilogue_row_mapping(gpu, mse, orc, nq):
    # only rows = p (mod 32) allowed, and every excluded row scores far above every allowed one: an epilogue that masks the wrong
    # accumulator takes an excluded row's score as its group's maximum, and the certificate (k-th exact score of the allowed rows
    # against that inflated maximum) fails -- so besides the answers, no query may need widening
    n = 2048
    qf = np.abs(orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq)))
    xf = np.abs(orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, n)))
    q = orc.f16_bits(qf)
    for p in range(32):
        allowed = (np.arange(n) % 32) == p
        base = orc.f16_bits(np.where(allowed[:, None], xf * 0.125, xf))
        vecs = mse.VectorList.from_f16s(base, D)
        s = mse.Searcher(vecs)
        sc, ids = s.bruteforce_topk(q, 1, mse.MODE_MFMA, allow=allowed)
        ws, wi = subset_oracle(orc, base, allowed, q, 1)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), p
        assert s.last_stats()["widened_queries"] == 0, p
        s.close()
        vecs.close()


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
def test_ties_by_lower_id(gpu, mse, orc, mode):
    n, nq, k = 3000, 12, 8
    base = orc.gen_rows_f16(SEED_BASE, 0, n).copy()
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    q[:, :] = base[7]                      # row 7 is every query's best match ...
    dup = [7, 100, 640, 2047, 2999]
    base[dup] = base[7]                   # ... and so are its copies
    mask = np.ones(n, bool)
    mask[[7, 640]] = False
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = run(mse, s, q, k, mode, mask)
    ws, wi = subset_oracle(orc, base, mask, q, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert list(ids[0, :3]) == [100, 2047, 2999]


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
def test_saturated_allowed_rows_rank_ahead_of_excluded(gpu, mse, orc, mode):
    # rows of f16 -v (v >= 500) against a query of 4096: the dot is below -2^31, its fixed-point score saturates to INT64_MIN (Rust
    # `as i64`).  625 groups, far more than the k + 8 the first round nominates; the saturated rows' values vary and the LOWEST ids
    # are the most negative, so their groups are never nominated first -- yet they must win the INT64_MIN tie by id
    n, nq, k = 20000, 10, 20
    base = orc.gen_rows_f16(SEED_BASE, 0, n).copy()
    r = np.arange(n)
    sat = r % 7 == 0
    vals = -4096.0 + (4096.0 - 500.0) * np.arange(sat.sum()) / sat.sum()    # -4096 (id 0) .. -500: dots -1.9e10 .. -2.4e9
    base[sat] = orc.f16_bits(np.repeat(vals[:, None], D, axis=1).astype(np.float32))
    q = orc.f16_bits(np.full((nq, D), 4096.0, np.float32))
    ordinary = np.flatnonzero(~sat)[::400][:12]              # 12 ordinary allowed rows; every other ordinary row excluded
    mask = sat.copy()
    mask[ordinary] = True
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = run(mse, s, q, k, mode, mask)
    ws, wi = subset_oracle(orc, base, mask, q, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert list(sc[0, -8:]) == [I64_MIN] * 8 and list(ids[0, -8:]) == list(range(0, 56, 7))
    assert not np.isin(ids, np.flatnonzero(~mask)).any()


def test_widening_under_a_filter(gpu, mse, orc):
    rng = np.random.default_rng(7)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 16)
    proto = orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, 1)[0])
    base_f = np.tile(proto, (3000, 1))
    flip = rng.integers(0, D, 3000)
    base_f[np.arange(3000), flip] *= (1.0 + 2.0 ** -9)
    base = orc.f16_bits(base_f)
    mask = rng.random(3000) < 0.5
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = subset_oracle(orc, base, mask, q, 10)
    sc, ids = s.bruteforce_topk(q, 10, mse.MODE_MFMA, allow=mask)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert s.last_stats()["widened_queries"] > 0


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_device_pointer_form_with_id_offset(gpu, mse, orc, mode):
    import torch
    n, nq, k, off = 9000, 40, 10, 123456
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    mask = np.random.default_rng(3).random(n) < 0.2
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    qd = torch.from_numpy(q.view(np.int16)).cuda()
    sd = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    idd = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    f = mse.RowFilter(mask)
    s.bruteforce_topk_dev(qd.data_ptr(), nq, k, sd.data_ptr(), idd.data_ptr(), MODES[mode], off, allow=f)
    mse.ffi.check(mse.ffi.lib().mse_device_synchronize())
    ws, wi = subset_oracle(orc, base, mask, q, k)
    got_i = idd.cpu().numpy().view(np.uint32)
    assert np.array_equal(sd.cpu().numpy(), ws)
    assert np.array_equal(got_i, np.where(wi == ID_NONE, ID_NONE, wi + off).astype(np.uint32))


@pytest.mark.parametrize("mode", ["exact", "mfma", "auto"])
def test_filter_shorter_than_base(gpu, mse, orc, mode):
    n, nf, nq, k = 5000, 3001, 130, 20
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    fmask = np.ones(nf, bool)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = run(mse, s, q, k, mode, mse.RowFilter(fmask))
    full = np.zeros(n, bool)
    full[:nf] = True
    ws, wi = subset_oracle(orc, base, full, q, k)
    assert np.array_equal(ids, wi) and np.array_equal(sc, ws)
    assert (ids < nf).all()
    with pytest.raises(mse.MseError):
        s.bruteforce_topk(q, k, MODES[mode], allow=np.ones(n + 1, bool))   # longer than the base


def test_filter_from_ids_equals_from_bits(gpu, mse, orc):
    n = 70000
    rng = np.random.default_rng(11)
    ids = rng.integers(0, n, 5000)
    ids = np.concatenate([ids, ids[:100]])             # duplicates allowed
    mask = np.zeros(n, bool)
    mask[ids] = True
    fa, fb = mse.RowFilter(ids, n_rows=n), mse.RowFilter(mask)
    assert len(fa) == len(fb) == n and fa.count == fb.count == int(mask.sum())
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 20)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    a = s.bruteforce_topk(q, 10, mse.MODE_MFMA, allow=fa)
    b = s.bruteforce_topk(q, 10, mse.MODE_EXACT, allow=fb)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def blocks_mask(n, starts, width):
    m = np.zeros(n, bool)
    for st in starts:
        m[st:st + width] = True
    return m


def blocks_rows(orc, starts, width):
    return np.concatenate([orc.gen_rows_f16(SEED_BASE, int(st), width) for st in sorted(starts)])


@pytest.mark.parametrize("count,nq", [(100, 1), (100, 300), (100000, 4), (100000, 40), (500000, 9)])
def test_sparse_path_and_scan_path_at_1e6(gpu, mse, orc, count, nq):
    # allowed rows in whole blocks, so that the oracle generates only them; together the cases lie on both sides of the crossover
    n, k = 1_000_000, 10
    width = min(count, 10000)
    starts = np.random.default_rng(count).choice(n // width, count // width, replace=False) * width
    mask = blocks_mask(n, starts, width)
    assert int(mask.sum()) == count
    s = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    f = mse.RowFilter(mask)
    rows = blocks_rows(orc, starts, width)
    ws, wi = orc.bruteforce_topk(rows, q, k)
    allowed = np.flatnonzero(mask)
    wi = allowed[wi].astype(np.uint32)
    for mode in ("exact", "mfma", "auto"):
        sc, ids = run(mse, s, q, k, mode, f)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), mode


def test_sparse_filter_at_1e7(gpu, mse, orc):
    n, count, width, nq, k = 10_000_000, 100_000, 10_000, 8, 10
    starts = np.random.default_rng(5).choice(n // width, count // width, replace=False) * width
    mask = blocks_mask(n, starts, width)
    s = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    ws, wi = orc.bruteforce_topk(blocks_rows(orc, starts, width), q, k)
    wi = np.flatnonzero(mask)[wi].astype(np.uint32)
    for mode in ("auto", "mfma"):
        sc, ids = run(mse, s, q, k, mode, mask)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), mode


def test_errors_write_nothing(gpu, mse, orc):
    lib = mse.ffi.lib()
    n, nq = 1000, 3
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = np.ascontiguousarray(orc.gen_rows_f16(SEED_QUERY, 0, nq))
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    f = mse.RowFilter(np.ones(n, bool))
    sc = np.full((nq, 2000), 7, np.int64)
    ids = np.full((nq, 2000), 7, np.uint32)
    qp = q.ctypes.data_as(C.POINTER(C.c_uint16))
    sp, ip = sc.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.mse_bruteforce_topk_filtered_f16(s._h, None, qp, nq, 10, 0, sp, ip) == -1
    assert b"null filter" in lib.mse_last_error()
    assert lib.mse_bruteforce_topk_filtered_f16(s._h, f._h, qp, nq, 1985, 0, sp, ip) == -1
    assert b"k too large" in lib.mse_last_error()
    assert (sc == 7).all() and (ids == 7).all()
    bad = np.array([1, 5, n], np.uint32)
    assert not lib.mse_filter_from_ids(bad.ctypes.data_as(C.POINTER(C.c_uint32)), 3, n)
    assert b"not below n_rows" in lib.mse_last_error()
    with pytest.raises(mse.MseError):
        mse.RowFilter(bad, n_rows=n)
    idx = mse.ScalarQuantizerIndex(D)
    idx.add(orc.f16_to_f32(base))
    dist = np.full((1, 10), 7, np.float32)
    lab = np.full((1, 10), 7, np.int64)
    qf = np.ascontiguousarray(orc.f16_to_f32(q[:1]))
    args = (qf.ctypes.data_as(C.POINTER(C.c_float)), 1, 10, dist.ctypes.data_as(C.POINTER(C.c_float)), lab.ctypes.data_as(C.POINTER(C.c_int64)))
    assert lib.mse_index_search_filtered(idx._h, None, *args) == -1
    assert b"null filter" in lib.mse_last_error()
    assert (dist == 7).all() and (lab == 7).all()
    idx.close()


def run_threads(n, fn):
    import threading
    out = [None] * n
    bar = threading.Barrier(n)

    def body(i):
        bar.wait()
        out[i] = fn(i)
    th = [threading.Thread(target=body, args=(i,)) for i in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def test_coalesced_requests_grouped_by_filter(gpu, mse, orc):
    # 64 threads x one query: a third with filter A, a third with B, a third unfiltered; each answer equals the call made alone
    n, T, k = 30000, 64, 10
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 0, T)
    rng = np.random.default_rng(21)
    fa, fb = mse.RowFilter(rng.random(n) < 0.3), mse.RowFilter(rng.random(n) < 0.7)
    pick = [fa, fb, None]
    vl = mse.VectorList.from_f16s(base, D)
    s = mse.Searcher(vl)
    alone = [s.bruteforce_topk(q[i:i + 1], k, mse.MODE_EXACT, allow=pick[i % 3]) for i in range(T)]
    disp = mse.Dispatcher(vl, max_wait_us=20000)
    got = run_threads(T, lambda i: disp.search(q[i], k, allow=pick[i % 3]))
    for i in range(T):
        assert np.array_equal(got[i][0], alone[i][0]) and np.array_equal(got[i][1], alone[i][1]), i
    st = disp.stats()
    assert st["requests"] == T and st["passes"] < T
    # the base's own coalescer (MODE_AUTO host calls of one pass) gives the same answers
    got = run_threads(T, lambda i: s.bruteforce_topk(q[i], k, mse.MODE_AUTO, allow=pick[i % 3]))
    for i in range(T):
        assert np.array_equal(got[i][0][0], alone[i][0][0]) and np.array_equal(got[i][1][0], alone[i][1][0]), i
    disp.close()


def index_of(mse, rows_f32):
    idx = mse.ScalarQuantizerIndex(D)
    idx.add(rows_f32)
    return idx


def mapped(res, allowed):
    lab = np.where(res.labels < 0, -1, allowed[np.maximum(res.labels, 0)])
    return res.distances, lab


@pytest.mark.parametrize("nq,k", [(3, 10), (40, 10), (300, 5), (9, 100)])
def test_flat_index_filtered_equals_index_of_allowed_rows(gpu, mse, orc, nq, k):
    n = 12000
    rng = np.random.default_rng(nq)
    x = orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, n)) * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq)) + np.float32(1e-3)
    for density in (0.0, 0.002, 0.5, 1.0):
        mask = rng.random(n) < density
        allowed = np.flatnonzero(mask)
        idx = index_of(mse, x)
        got = idx.search(qf, k, allow=mask)
        if allowed.size:
            sub = index_of(mse, x[allowed])
            wd, wl = mapped(sub.search(qf, k), allowed)
            sub.close()
        else:
            wd, wl = np.full((nq, k), -np.finfo(np.float32).max, np.float32), np.full((nq, k), -1, np.int64)
        assert np.array_equal(got.labels, wl), density
        assert np.array_equal(got.distances.view(np.uint32), wd.view(np.uint32)), density
        idx.close()


def test_flat_index_old_filter_excludes_added_rows(gpu, mse, orc):
    n0, n1, nq, k = 5000, 3000, 20, 10
    x = orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, n0 + n1))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, nq))
    idx = index_of(mse, x[:n0])
    f = mse.RowFilter(np.ones(n0, bool))
    before = idx.search(qf, k, allow=f)
    idx.add(x[n0:] * 4.0)          # new rows that would outscore every old one
    after = idx.search(qf, k, allow=f)
    assert (after.labels < n0).all()
    assert np.array_equal(after.labels, before.labels) and np.array_equal(after.distances, before.distances)
    unfiltered = idx.search(qf, k)
    assert (unfiltered.labels >= n0).any()
    with pytest.raises(mse.MseError):
        idx.search(qf, k, allow=np.ones(n0 + n1 + 1, bool))   # longer than the index
    idx.close()


def test_flat_index_coalesced_requests_grouped_by_filter(gpu, mse, orc):
    n, T, k = 20000, 64, 10
    x = orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, n))
    qf = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, T))
    rng = np.random.default_rng(5)
    fa, fb = mse.RowFilter(rng.random(n) < 0.3), mse.RowFilter(rng.random(n) < 0.7)
    pick = [fa, fb, None]
    idx = index_of(mse, x)
    alone = [idx.search(qf[i], k, allow=pick[i % 3]) for i in range(T)]
    st0 = idx.stats()
    got = run_threads(T, lambda i: idx.search(qf[i], k, allow=pick[i % 3]))
    for i in range(T):
        assert np.array_equal(got[i].labels, alone[i].labels), i
        assert np.array_equal(got[i].distances.view(np.uint32), alone[i].distances.view(np.uint32)), i
    st = idx.stats()
    assert st["requests"] - st0["requests"] == T and st["passes"] - st0["passes"] < T
    idx.close()
