"""The 320-query pass of the matrix-core scan writes ONE group maximum per 64 rows (the rows one wave owns), where every other pass writes
one per 32 (scan_mfma.hip scan_mfma2d_kernel GR = 64, bruteforce.hip mfma_pass).  Pinned down here at 257 and 320 queries, the counts that take
that pass: bases that are whole tiles, that end 1 .. 255 rows into a tile (on either side of a 32- and a 64-row group boundary) and that
are smaller than one tile; the widening, which then re-scores 64-row groups; filters seen from a 64-row group (one allowed row, none,
allowed rows in its second half only); the debug hook, which must go on returning 32-row maxima; and two shards on one device.
Every answer is compared with the exact mode and the oracle: ids and i64 scores equal."""
import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152
EPS = 2.8e-4   # bruteforce.hip mfma_pass -> launch_query_eps: |matrix-core score - exact-order score| <= EPS * |q| * max |x|


def check_both_modes(mse, orc, base, q, k):
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = orc.bruteforce_topk(base, q, k)
    sm, im = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert np.array_equal(im, wi) and np.array_equal(sm, ws)
    se, ie = s.bruteforce_topk(q, k, mse.MODE_EXACT)
    assert np.array_equal(ie, im) and np.array_equal(se, sm)
    return s


def subset_oracle(orc, base, mask, q, k):
    """the oracle over base[mask], ids mapped back; slots past the allowed rows stay (INT64_MIN, ID_NONE) as the library leaves them"""
    allowed = np.flatnonzero(mask)
    ws = np.full((len(q), k), np.iinfo(np.int64).min, np.int64)
    wi = np.full((len(q), k), 0xFFFFFFFF, np.uint32)
    m = min(k, len(allowed))
    if m:
        s, i = orc.bruteforce_topk(base[allowed], q, m)
        ws[:, :m], wi[:, :m] = s, allowed[i].astype(np.uint32)
    return ws, wi


# whole tiles (1024, 5120), ragged tails of 1, 31, 33, 63, 65 and 255 rows after 1024, and bases below one 256-row tile
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("n", [1024, 5120, 1025, 1055, 1057, 1087, 1089, 1279, 1, 63, 64, 65, 200])
def test_whole_tiles_ragged_tails_and_small_bases(gpu, mse, orc, n, nq):
    assert mse.ffi.lib().mse_queries_per_pass_max(D) == 320
    base = orc.gen_rows_f16(SEED_BASE, 17, n)
    q = orc.gen_rows_f16(SEED_QUERY, 17, nq)
    check_both_modes(mse, orc, base, q, min(10, n))


# enough groups that the first round cannot take them all (18 of them: 1152 rows), the last one ragged
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("n", [40 * 256, 40 * 256 + 33, 40 * 256 + 65])
def test_more_groups_than_the_first_round_takes(gpu, mse, orc, n, nq):
    base = orc.gen_rows_f16(SEED_BASE, 19, n)
    q = orc.gen_rows_f16(SEED_QUERY, 19, nq)
    s = check_both_modes(mse, orc, base, q, 10)
    s.bruteforce_topk(q, 10, mse.MODE_MFMA)               # the counters of the MFMA call (the exact mode resets them)
    assert s.last_stats()["max_groups"] >= 18             # groups are still counted as groups: k + 8 = 18 in the first round


# near-duplicates of one row around every query's k-th score: the certificate fails and the widening runs from 64-row groups
@pytest.mark.parametrize("nq", [257, 320])
def test_widening_from_64_row_groups(gpu, mse, orc, nq):
    rng = np.random.default_rng(23)
    n = 6000 + 37
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    proto = orc.f16_to_f32(orc.gen_rows_f16(SEED_BASE, 0, 1)[0])
    base_f = np.tile(proto, (n, 1))
    base_f[np.arange(n), rng.integers(0, D, n)] *= (1.0 + 2.0 ** -9)
    base = orc.f16_bits(base_f)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = orc.bruteforce_topk(base, q, 10)
    sm, im = s.bruteforce_topk(q, 10, mse.MODE_MFMA)
    st = s.last_stats()
    assert np.array_equal(im, wi) and np.array_equal(sm, ws)
    assert st["widened_queries"] > 0 and st["max_groups"] > 18, st
    se, ie = s.bruteforce_topk(q, 10, mse.MODE_EXACT)
    assert np.array_equal(ie, im) and np.array_equal(se, sm)


def _filters(n, rng):
    one = np.zeros(n, bool)                 # exactly one allowed row in every 64-row group, anywhere in it
    starts = np.arange(0, n, 64)
    one[np.minimum(starts + rng.integers(0, 64, len(starts)), n - 1)] = True
    some_empty = rng.random(n) < 0.5        # every third 64-row group has no allowed row at all
    for g in range(0, len(starts), 3):
        some_empty[starts[g]:starts[g] + 64] = False
    second_half = np.zeros(n, bool)         # allowed rows only in rows 32 .. 63 of their 64-row group
    second_half[(np.arange(n) % 64) >= 32] = rng.random(int(((np.arange(n) % 64) >= 32).sum())) < 0.4
    return {"one_row_per_group": one, "empty_groups": some_empty, "second_half_only": second_half}


@pytest.mark.parametrize("kind", ["one_row_per_group", "empty_groups", "second_half_only"])
@pytest.mark.parametrize("n", [4096, 4096 + 97])
def test_filtered_320(gpu, mse, orc, kind, n):
    rng = np.random.default_rng(n)
    mask = _filters(n, rng)[kind]
    base = orc.gen_rows_f16(SEED_BASE, 29, n)
    q = orc.gen_rows_f16(SEED_QUERY, 29, 320)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = subset_oracle(orc, base, mask, q, 10)
    f = mse.RowFilter(mask)
    for mode in (mse.MODE_MFMA, mse.MODE_EXACT):
        sc, ids = s.bruteforce_topk(q, 10, mode, allow=f)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), mode
    real = ids[ids != 0xFFFFFFFF]
    assert mask[real].all()


# the debug hook is read as 32-row maxima by the older tests and keeps returning exactly that at 320 queries
@pytest.mark.parametrize("n", [2048, 2048 + 65, 97])
def test_debug_group_max_stays_32_rows(gpu, mse, orc, n):
    from mse import ffi
    nq = 320
    base = orc.gen_rows_f16(SEED_BASE, 31, n)
    q = orc.gen_rows_f16(SEED_QUERY, 31, nq)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    s.bruteforce_topk(q, min(10, n), mse.MODE_MFMA)       # a 64-row pass first: the hook must not inherit its layout
    n_groups = (n + 31) // 32
    got = np.full((n_groups, nq), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_mfma_group_max(s._h, q.ctypes.data_as(ffi.u16p), nq, got.ctypes.data_as(ffi.f32p)))
    x64, q64 = orc.f16_to_f32(base).astype(np.float64), orc.f16_to_f32(q).astype(np.float64)
    dots = x64 @ q64.T
    pad = np.full((n_groups * 32 - n, nq), -np.inf)
    want = np.concatenate([dots, pad]).reshape(n_groups, 32, nq).max(axis=1)
    bound = EPS * np.linalg.norm(q64, axis=1) * np.linalg.norm(x64, axis=1).max()
    err = np.abs(got.astype(np.float64) - want)
    print("max |32-row group max - float64| / bound =", float((err / bound).max()))
    assert np.all(err <= bound), np.argwhere(~(err <= bound))[:8]


def test_two_shards_on_one_device_320(gpu, mse, orc):
    n, nq, k = 9000 + 41, 320, 10
    q = orc.gen_rows_f16(SEED_QUERY, 37, nq)
    whole = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    ws, wi = whole.bruteforce_topk(q, k, mse.MODE_MFMA)
    os_, oi = orc.bruteforce_topk(orc.gen_rows_f16(SEED_BASE, 0, n), q, k)
    assert np.array_equal(wi, oi) and np.array_equal(ws, os_)
    grp = mse.ShardGroup(2, D, devices=[0, 0])
    grp.generate(SEED_BASE, 0, n)
    for mode in (mse.MODE_MFMA, mse.MODE_EXACT):
        s, i = grp.bruteforce_topk(q, k, mode)
        assert np.array_equal(i, wi) and np.array_equal(s, ws), mode
    grp.close()
