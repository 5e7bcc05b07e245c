"""The 320-query pass of the matrix-core scan on the two-dimensional wave split (scan_mfma.hip, scan_mfma2d_kernel at BN = 320: a wave owns
64 rows x 160 queries).  What that tiling can get wrong and the older tests do not pin down at 320 queries: ragged row counts around one
and two tiles per workgroup, both query halves with and without the padding columns, a filter that ends inside a 32-row group, several
full passes in one launch, and the raw group maxima column by column (the one check that sees a column written to the wrong query
before the certificate repairs it by widening)."""
import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152
EPS = 2.8e-4   # bruteforce.hip mfma_pass -> launch_query_eps: |matrix-core score - exact-order score| <= EPS * |q| * max |x|


def subset_oracle(orc, base, mask, q, k):
    """orc.bruteforce_topk over base[mask], ids mapped through flatnonzero(mask) (as in test_gpu_filtered.py; >= k rows allowed here)."""
    allowed = np.flatnonzero(mask)
    ws, wi = orc.bruteforce_topk(base[allowed], q, k)
    return ws, allowed[wi].astype(np.uint32)


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_both_modes(mse, orc, base, q, k, d=D):
    s = mse.Searcher(mse.VectorList.from_f16s(base, d))
    ws, wi = orc.bruteforce_topk(base, q, k)
    sm, im = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert np.array_equal(im, wi) and np.array_equal(sm, ws)
    se, ie = s.bruteforce_topk(q, k, mse.MODE_EXACT)
    assert np.array_equal(ie, im) and np.array_equal(se, sm)
    return s


# (a) + (b): rows that are no multiple of 256 or 32, around one tile; queries 257..320 present and absent
@pytest.mark.parametrize("nq", [257, 289, 320])
@pytest.mark.parametrize("n", [31, 33, 255, 257, 289, 511, 545, 4097])
def test_ragged_rows_and_query_halves(gpu, mse, orc, n, nq):
    assert mse.ffi.lib().mse_queries_per_pass_max(D) == 320
    base = orc.gen_rows_f16(SEED_BASE, 7, n)
    q = orc.gen_rows_f16(SEED_QUERY, 7, nq)
    check_both_modes(mse, orc, base, q, min(10, n))


# (a): one and two tiles per workgroup (the grid is one workgroup per CU), the last tile ragged; d = 128 is the shortest
# two-stage ring (two K blocks: every block is the first or the last of its tile)
@pytest.mark.parametrize("tiles,extra,d,nq", [(1, 33, 1152, 320), (1, -31, 1152, 289), (2, 33, 128, 320), (2, -223, 128, 257), (1, 1, 128, 320)])
def test_one_and_two_tiles_per_workgroup(gpu, mse, orc, tiles, extra, d, nq):
    n = tiles * 256 * n_cu() + extra
    base = orc.gen_rows_f16(SEED_BASE, 11, n, d)
    q = orc.gen_rows_f16(SEED_QUERY, 11, nq, d)
    check_both_modes(mse, orc, base, q, 10, d)


# (c): a filter whose bitmap ends inside a 32-row group (shorter than the base, and as long as a ragged base)
@pytest.mark.parametrize("n,nf,nq", [(5000, 3001, 320), (5000, 2575, 289), (1301, 1301, 320), (600, 257, 257)])
def test_filter_ending_mid_group(gpu, mse, orc, n, nf, nq):
    rng = np.random.default_rng(n + nf)
    base = orc.gen_rows_f16(SEED_BASE, 3, n)
    q = orc.gen_rows_f16(SEED_QUERY, 3, nq)
    fmask = rng.random(nf) < 0.5
    fmask[nf - 1] = True                                   # the last bit of the bitmap is a live row
    full = np.zeros(n, bool)
    full[:nf] = fmask
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = subset_oracle(orc, base, full, q, 10)
    for mode in (mse.MODE_MFMA, mse.MODE_EXACT):
        sc, ids = s.bruteforce_topk(q, 10, mode, allow=mse.RowFilter(fmask))
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), mode
    assert (ids < nf).all()


# (d): a small base with three full 320-query passes side by side in one launch
def test_three_full_passes_in_one_launch(gpu, mse, orc):
    base = orc.gen_rows_f16(SEED_BASE, 5, 4096)
    q = orc.gen_rows_f16(SEED_QUERY, 5, 960)
    check_both_modes(mse, orc, base, q, 5)


# (e): the raw group maxima of one 320-query pass against the float64 maximum of the exact dots of each 32-row group
@pytest.mark.parametrize("n,nq", [(845, 320), (257, 257), (256 * 3 + 31, 289), (20001, 320)])
def test_group_maxima_column_by_column(gpu, mse, orc, n, nq):
    from mse import ffi
    base = orc.gen_rows_f16(SEED_BASE, 13, n)
    q = orc.gen_rows_f16(SEED_QUERY, 13, nq)
    q[::3] = orc.f16_bits(orc.f16_to_f32(q[::3]) * np.float32(2.5))   # columns of different scale: a swapped column is far outside the bound
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    n_groups = (n + 31) // 32
    got = np.empty((n_groups, nq), np.float32)
    ffi.check(ffi.lib().mse_debug_mfma_group_max(s._h, q.ctypes.data_as(ffi.u16p), nq, got.ctypes.data_as(ffi.f32p)))
    x64, q64 = orc.f16_to_f32(base).astype(np.float64), orc.f16_to_f32(q).astype(np.float64)
    dots = x64 @ q64.T                                                # [n][nq]
    pad = np.full((n_groups * 32 - n, nq), -np.inf)
    want = np.concatenate([dots, pad]).reshape(n_groups, 32, nq).max(axis=1)
    bound = EPS * np.linalg.norm(q64, axis=1) * np.linalg.norm(x64, axis=1).max()
    err = np.abs(got.astype(np.float64) - want)
    print("max |group max - float64| / bound =", float((err / bound).max()))
    assert np.all(err <= bound), np.argwhere(err > bound)[:8]


# the certificate's work on the bench's own data: a tiling bug that only costs widenings would otherwise hide as a slowdown
def test_widenings_do_not_exceed_those_of_the_untouched_kernels(gpu, mse, orc):
    n, k = 1_000_000, 10
    s = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    q = orc.gen_rows_f16(SEED_QUERY, 0, 320)
    s320, i320 = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    w320 = s.last_stats()["widened_queries"]
    s256, i256 = s.bruteforce_topk(q[:256], k, mse.MODE_MFMA)
    w256 = s.last_stats()["widened_queries"]
    s64, i64 = s.bruteforce_topk(q[256:], k, mse.MODE_MFMA)
    w64 = s.last_stats()["widened_queries"]
    print("widened queries: 320-query call", w320, "| 256-query call", w256, "+ 64-query call", w64)
    assert np.array_equal(i320, np.concatenate([i256, i64])) and np.array_equal(s320, np.concatenate([s256, s64]))
    assert w320 <= w256 + w64
