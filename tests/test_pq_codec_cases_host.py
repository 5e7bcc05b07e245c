"""The cases of tests/pq_codec_cases.py against the oracle alone: each one is what its comment says it is -- the planted ties give the
planted codes, the tables are sensitive to the order of their adds, the rounding list rounds as integer arithmetic says, the saturated
score model is saturated.  No device is needed; tests/test_gpu_pq_codec_edges.py runs the same cases on one."""
import numpy as np
import pytest

import pq_codec_cases as cases


@pytest.mark.parametrize("d,dpc", cases.TRANSFORM_SHAPES)
def test_transform_is_neither_symmetric_nor_orthonormal(orc, d, dpc):
    c = cases.transform_case(orc, d, dpc)
    T, x = c["T"].astype(np.float64), c["x"].astype(np.float64)
    assert d % dpc == 0 and c["x"].shape == (max(cases.TRANSFORM_BATCHES), d)
    right, wrong = x @ T.T, x @ T
    rel = np.linalg.norm(right - wrong, axis=1) / np.linalg.norm(right, axis=1)
    assert rel.min() > 1e-2, rel.min()                       # a transposed read is no rounding error, for every test vector
    assert np.abs(T @ T.T - np.eye(d)).max() > 0.5
    # the oracle's k-ascending f32 chain is the product it claims to be
    assert np.allclose(c["want"], right, rtol=0, atol=1e-5 * np.abs(right).max())


@pytest.mark.parametrize("d,dpc", [(90, 18), (64, 16)])
def test_planted_ties_give_the_planted_codes(orc, d, dpc):
    cents, T, x, want = cases.planted_tie_case(d, dpc)
    got = orc.PQ(cents, T, dpc, d).quantize_batch(x)
    assert np.array_equal(got, want)
    assert np.array_equal(cents[1], cents[3]) and np.array_equal(cents[2], cents[4]) and np.array_equal(cents[2], cents[5])
    assert list(got[0]) == [1] * (d // dpc) and list(got[1]) == [2] * (d // dpc)      # lowest index of two, of three equal centroids
    assert not got[2].any() and not x[2].any()                                        # every product zero
    assert np.isnan(x[3, dpc:2 * dpc]).all() and not np.isnan(x[3, :dpc]).any() and not got[3].any()
    cents, T, x, want = cases.planted_tie_case(d, dpc, with_inf=True)
    assert np.all(cents[0, dpc:2 * dpc] == -np.inf) and np.all(x > 0)
    assert np.array_equal(orc.PQ(cents, T, dpc, d).quantize_batch(x), want) and np.all(want == 1)


def test_quantize_cases_use_every_centroid_count(orc):
    for nc in cases.TILED_CENTROIDS:
        c = cases.quantize_case(orc, 90, 18, nc, max(cases.TILED_BATCHES))
        assert c["want"].shape == (2049, 5) and c["want"].max() == nc - 1 and c["cents"].shape == (nc, 90)
    for d, dpc in cases.GENERIC_SHAPES:
        assert d % dpc == 0 and dpc != 18


@pytest.mark.parametrize("d,dpc,nc", cases.QUANTIZE_BASE_SHAPES)
def test_f16_edge_rows_hold_subnormals_and_the_largest_values(orc, d, dpc, nc):
    rows = cases.f16_edge_rows(orc, d)
    assert rows.shape == (300, d) and d % 64 == 0 and d % dpc == 0
    mag = rows & 0x7FFF
    assert np.sum((mag > 0) & (mag < 0x400) & (rows < 0x8000)) > 50 and np.sum((mag > 0) & (mag < 0x400) & (rows >= 0x8000)) > 50
    assert np.sum(rows == 0x7BFF) >= 30 and np.sum(rows == 0xFBFF) >= 30 and mag.max() == 0x7BFF       # finite throughout
    assert np.all(np.isfinite(orc.f16_to_f32(rows)))


@pytest.mark.parametrize("n_chunks,nc", [(64, 256), (64, 16)] + [(c, k) for c in cases.FULL_SCAN_CHUNKS for k in cases.FULL_SCAN_CENTROIDS])
def test_tables_show_the_order_of_their_adds(orc, n_chunks, nc):
    lut = cases.wide_table(n_chunks, nc)
    mag = np.abs(lut)
    assert (lut > 0).any() and (lut < 0).any() and mag.min() >= 2.0 ** -20 * 0.999 and mag.max() <= 8.0
    if lut.size >= 256:
        assert mag.min() < 2.0 ** -17 and mag.max() > 1.0
    codes = cases.random_codes(cases.GATHER_ROWS, n_chunks, nc)
    assert codes.max() < nc
    opq = orc.PQ(*cases.adc_codec(n_chunks, nc))
    fwd, rev = opq.asymmetric_dot_product(lut, codes), cases.reversed_sums(opq, lut, codes)
    assert np.mean(fwd != rev) >= 0.1, np.mean(fwd != rev)
    exact = lut.astype(np.float64)[np.arange(n_chunks)[None, :], codes].sum(axis=1) * 2.0 ** 32
    assert np.abs(fwd - exact).max() <= n_chunks * 2.0 ** -24 * 8.0 * n_chunks * 2.0 ** 32


def test_adc_shapes_reach_the_paths_they_name():
    assert [(c * 3) & 3 for c in cases.FULL_SCAN_CHUNKS].count(0) < len(cases.FULL_SCAN_CHUNKS)     # a scalar table copy occurs
    assert all((c * 256) & 3 == 0 for c in cases.FULL_SCAN_CHUNKS)
    assert [c % 16 == 0 for c in cases.FULL_SCAN_CHUNKS] == [True, True, False, False]
    assert min(cases.FULL_SCAN_BATCHES) == 1 and {255, 256, 1023, 1024, 1025} <= set(cases.FULL_SCAN_BATCHES)
    assert cases.FRESH_SCAN_BATCHES[0] == 65
    for cu in (64, 256, 304):
        assert cases.second_group_rows(cu) > 64 * 16 * cu and cases.second_group_rows(cu) % 64 != 0
        assert cases.second_trip_ids(cu) > 2 * cu * 1024 * 4 and cases.second_trip_ids(cu) % 4 != 0
    ids, bad = cases.bad_ids()
    assert set(ids[bad].tolist()) == {cases.GATHER_ROWS, 0xFFFFFFFF} and ids[~bad].max() < cases.GATHER_ROWS
    assert len(np.unique(ids[~bad])) < (~bad).sum()                                                  # repeats
    for n_chunks, nc, nd in cases.DESC_SHAPES:
        desc, sc = cases.descriptors(cases.GATHER_ROWS, nd), cases.mixed_scales(nd)
        assert desc.shape == (cases.GATHER_ROWS, nd) and (desc == 0).any() and (desc == 255).any()
        assert sc.size == nd and (sc > 0).any() and (sc < 0).any()


@pytest.mark.parametrize("n", cases.RANK_ROWS)
def test_rank_cases_are_ruled_by_ties(orc, n):
    base, query = cases.rank_base(orc, n)
    assert base.shape == (n, cases.RANK_D)
    scores = orc.score_all(base, query)
    vals, counts = np.unique(scores, return_counts=True)
    shared = np.isin(scores, vals[counts > 1])
    ranks = orc.ranks_from_scores(scores)
    assert sorted(ranks.tolist()) == list(range(n))
    for m in cases.RANK_TARGETS:
        t = cases.rank_targets(n, m)
        assert t.size == m and t.max() < n
        if m >= 7:
            assert 0 in t and n - 1 in t and np.sum(t == n // 2) >= 5
        if n > 1:           # (a base of one row has no other row to share a score with)
            assert np.mean(shared[t]) >= 1 / 3, (n, m, np.mean(shared[t]))
    if n > 1:
        # equal scores: the lower id ranks first
        i = np.flatnonzero(shared)
        first = i[0]
        twin = np.flatnonzero(scores == scores[first])
        assert len(twin) > 1 and np.array_equal(ranks[twin], ranks[twin[0]] + np.arange(len(twin)))


def test_rounding_list_rounds_as_the_integers_say(orc):
    f32_bits, want = cases.f16_rounding_list()
    assert f32_bits.size == want.size == 2 * 48 * 64 and len(cases.f16_patterns()) == 1023 == len(set(cases.f16_patterns()))
    x = f32_bits.view(np.float32)
    assert np.all(np.isfinite(x)) and (want & 0x7FFF).max() == 0x7BFF
    assert np.array_equal(orc.f16_bits(x), want)
    pats = np.array(cases.f16_patterns())
    assert (pats < 0x400).sum() >= 100 and ((pats >= 0x3F0) & (pats < 0x410)).sum() == 32 and (pats >= 0x7800).sum() >= 128
    assert len(np.unique(pats >> 10)) == 31                                        # every exponent of the format
    # the three named values
    assert x[6138] == 2.0 ** -25 and want[6138] == 0 and want[6139] == 1
    assert x[6140] == np.nextafter(np.float32(65520.0), np.float32(0)) and want[6140] == 0x7BFF
    # a midpoint really is one: numpy's own conversion (also round-half-even) agrees, and so do the neighbours
    assert np.array_equal(x.astype(np.float16).view(np.uint16), want)
    pats16 = pats.astype(np.uint16)
    lo, hi = orc.f16_to_f32(pats16).astype(np.float64), orc.f16_to_f32(pats16 + 1).astype(np.float64)
    assert np.array_equal(x[0:6138:6].astype(np.float64), (lo + hi) / 2)


@pytest.mark.parametrize("shape", cases.SCORE_SHAPES)
def test_score_model_cases(orc, shape):
    up, bias, down, x = cases.score_case(shape, saturated=True)
    pre = cases.pre_activations_f64(up, bias, x)
    assert np.all((pre >= 21.0) | (pre <= -111.0)), (pre.min(), pre.max())
    if shape[1] > 1:
        assert (pre >= 21.0).any() and (pre <= -111.0).any()
    got = orc.score_batch(up, bias, down, x)
    assert got.shape == (shape[3], shape[2]) and np.all(np.isfinite(got))
    # saturated: silu is the identity or zero, so the oracle equals the f64 restatement with silu replaced by that
    h = np.where(pre >= 21.0, pre, 0.0)
    want = h @ down.astype(np.float64).T * (shape[0] / shape[1])
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    up, bias, down, x = cases.score_case(shape, saturated=False)
    want = cases.score_batch_f64(up, bias, down, x)
    assert np.abs(want).max() < 8.0                                                 # outputs of order 1
    assert np.allclose(orc.score_batch(up, bias, down, x), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("cdf_len", cases.BUCKET_CDF_LENS)
@pytest.mark.parametrize("n_desc,n", cases.BUCKET_SHAPES)
def test_bucket_cases(orc, n_desc, n, cdf_len):
    cdfs = cases.bucket_cdfs(n_desc, cdf_len)
    assert cdfs.shape == (n_desc, cdf_len) and np.all(np.diff(cdfs, axis=1) >= 0) and np.all((cdfs == 0.0).any(axis=1))
    if cdf_len >= 254:
        for c in cdfs:
            assert c[0] == c[1] == c[2] < c[3] and c[99] < c[100] == c[103] < c[104] and c[-4] < c[-3] == c[-1]
    scores = cases.bucket_scores(cdfs, n)
    got = orc.descriptor_buckets(cdfs, scores)
    plain = ~np.isnan(scores) & ~cases.in_equal_run(cdfs, scores)
    for j in range(n_desc):
        want = np.searchsorted(cdfs[j], scores[:, j], "left")
        assert np.array_equal(got[plain[:, j], j], want[plain[:, j]])
    if n * n_desc >= 250:
        flat = scores.reshape(-1)
        assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any() and np.any((flat == 0) & np.signbit(flat))
        assert cdf_len == 1 or cases.in_equal_run(cdfs, scores).any()
        if cdf_len >= 254:
            assert plain.any() and np.any((scores < cdfs[:, 0][None, :]) & np.isfinite(scores)) and np.any((scores > cdfs[:, -1][None, :]) & np.isfinite(scores))
            assert np.any(np.isin(scores, cdfs) & plain)                           # equals a single entry
