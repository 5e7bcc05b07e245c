"""The kernels that encode an index and score codes (csrc/pq.hip: transform, table, quantise, ADC, conversions, rank count;
csrc/index_pack.hip: score model, descriptor buckets) against the oracle, route by route, at the sizes where each route begins or ends.
The cases come from tests/pq_codec_cases.py; tests/test_pq_codec_cases_host.py shows on the oracle alone that they are what they claim.
Everything is bit for bit -- the oracle and the kernels state the same summation orders -- except the unsaturated score model, which
is held to float64 within the tolerance its kernel states."""
import numpy as np
import pytest

import pq_codec_cases as cases

pytestmark = pytest.mark.gpu
I64_MIN = np.iinfo(np.int64).min


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- transform ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dpc", cases.TRANSFORM_SHAPES)
def test_batch_transform_both_kernels_every_ragged_tile(gpu, mse, orc, d, dpc):
    c = cases.transform_case(orc, d, dpc)
    gpq = mse.ProductQuantizer(c["cents"], c["T"], dpc, d)
    for n in cases.TRANSFORM_BATCHES:
        assert np.array_equal(gpq.apply_transform(c["x"][:n]), c["want"][:n]), n


@pytest.mark.parametrize("d,dpc", cases.TRANSFORM_SHAPES)
def test_query_transform_and_table(gpu, mse, orc, d, dpc):
    """preprocess_query: the one-vector kernel (64-, 8- and 1-wide loops over the transposed matrix), then the f64 table.  The table
    built by the oracle from the DEVICE's batch transform of the same query is the same table: the vector kernel and the batch kernels
    produce the same bits."""
    c = cases.transform_case(orc, d, dpc)
    gpq = mse.ProductQuantizer(c["cents"], c["T"], dpc, d)
    for row in (0, 5, 319):
        q = c["x"][row]
        table = gpq.preprocess_query(q).table
        assert table.shape == (d // dpc, 16)
        assert np.array_equal(table, c["opq"].preprocess_query(q)), row
        assert np.array_equal(table, c["opq"].lut_from_transformed(gpq.apply_transform(q[None, :])[0])), row


# ---- quantise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", cases.TILED_CENTROIDS)
@pytest.mark.parametrize("d", cases.TILED_WIDTHS)
def test_tiled_quantise_around_one_workgroup(gpu, mse, orc, d, nc):
    """dpc = 18: one workgroup owns 256 x 4 vectors of one chunk; vectors past n are clamped to row n - 1, computed and not stored."""
    ns = cases.tiled_batches(d)
    c = cases.quantize_case(orc, d, 18, nc, max(ns))
    gpq = mse.ProductQuantizer(c["cents"], c["T"], 18, d)
    for n in ns:
        assert np.array_equal(gpq.quantize_batch(c["x"][:n]), c["want"][:n]), n


@pytest.mark.parametrize("nc", cases.GENERIC_CENTROIDS)
@pytest.mark.parametrize("d,dpc", cases.GENERIC_SHAPES)
def test_generic_quantise(gpu, mse, orc, d, dpc, nc):
    c = cases.quantize_case(orc, d, dpc, nc, max(cases.GENERIC_BATCHES))
    gpq = mse.ProductQuantizer(c["cents"], c["T"], dpc, d)
    for n in cases.GENERIC_BATCHES:
        assert np.array_equal(gpq.quantize_batch(c["x"][:n]), c["want"][:n]), n


@pytest.mark.parametrize("d,dpc", [(90, 18), (64, 16)])
def test_quantise_planted_ties_nan_and_infinity(gpu, mse, orc, d, dpc):
    """Two and three identical centroids -> the lowest index; every product zero -> 0; NaN -> 0 (strict `>` from -inf never fires);
    a centroid sub-vector of -inf under positive input never wins.  The oracle gives exactly these codes (host test)."""
    for with_inf in (False, True):
        cents, T, x, want = cases.planted_tie_case(d, dpc, with_inf)
        got = mse.ProductQuantizer(cents, T, dpc, d).quantize_batch(x)
        assert np.array_equal(got, want), with_inf
        assert np.array_equal(got, orc.PQ(cents, T, dpc, d).quantize_batch(x)), with_inf


@pytest.mark.parametrize("d,dpc,nc", cases.QUANTIZE_BASE_SHAPES)
def test_quantize_base_on_f16_edge_rows(gpu, mse, orc, d, dpc, nc):
    """Codes.quantize_base: widening, transform and quantise without leaving the device, on rows with f16 subnormals and +-65504."""
    cents, T = cases.skewed_codec(orc, d, dpc, nc, seed=29)
    rows = cases.f16_edge_rows(orc, d)
    gpq = mse.ProductQuantizer(cents, T, dpc, d)
    codes = mse.Codes.quantize_base(gpq, mse.VectorList.from_f16s(rows, d))
    assert len(codes) == len(rows)
    want = orc.PQ(cents, T, dpc, d).quantize_batch(orc.f16_to_f32(rows))
    assert np.array_equal(codes.read_rows(0, len(rows)), want)
    assert np.array_equal(gpq.quantize_batch(orc.f16_to_f32(rows)), want)


# ---- ADC ----------------------------------------------------------------------------------------------------------------------------
def adc_pair(mse, orc, n_chunks, nc):
    shape = cases.adc_codec(n_chunks, nc)
    return orc.PQ(*shape), mse.ProductQuantizer(*shape)


@pytest.mark.parametrize("n", cases.FRESH_SCAN_BATCHES)
def test_full_scan_64x256_first_call_of_a_fresh_handle(gpu, mse, orc, n):
    """mse_pq_adc on a 64 x 256 codec is the group scan, which fetches whole groups of 64 code rows: its staging buffer carries a group
    of slack like every other code buffer.  The scan is the handle's FIRST call here, so no earlier call has grown that buffer; n = 65
    has one row in its last group."""
    opq, gpq = adc_pair(mse, orc, 64, 256)
    lut = cases.wide_table(64, 256)
    codes = cases.random_codes(n, 64, 256)
    assert np.array_equal(gpq.asymmetric_dot_product(lut, codes), opq.asymmetric_dot_product(lut, codes))


def test_full_scan_64x256_a_wave_takes_a_second_group(gpu, mse, orc):
    n = cases.second_group_rows(n_cu())
    opq, gpq = adc_pair(mse, orc, 64, 256)
    lut = cases.wide_table(64, 256)
    codes = cases.random_codes(n, 64, 256)
    assert np.array_equal(gpq.asymmetric_dot_product(lut, codes), opq.asymmetric_dot_product(lut, codes))


@pytest.mark.parametrize("nc", cases.FULL_SCAN_CENTROIDS)
@pytest.mark.parametrize("n_chunks", cases.FULL_SCAN_CHUNKS)
def test_full_scan_generic_bodies(gpu, mse, orc, n_chunks, nc):
    """Not 64 x 256: pq_adc_kernel without ids -- 16 code bytes at a time (16 | n_chunks) or byte by byte, the table copied as float4
    or scalar, workgroups of 256 (n < 1024) and 1024 threads."""
    opq, gpq = adc_pair(mse, orc, n_chunks, nc)
    lut = cases.wide_table(n_chunks, nc)
    codes = cases.random_codes(max(cases.FULL_SCAN_BATCHES), n_chunks, nc)
    want = opq.asymmetric_dot_product(lut, codes)
    for n in cases.FULL_SCAN_BATCHES:
        assert np.array_equal(gpq.asymmetric_dot_product(lut, codes[:n]), want[:n]), n


@pytest.mark.parametrize("nc", cases.GATHER_CENTROIDS)
def test_gathered_fast_path(gpu, mse, orc, nc):
    """64 chunks with ids: four ids per thread and trip, the next trip's ids in flight.  The table row stride is n_centroids."""
    opq, gpq = adc_pair(mse, orc, 64, nc)
    lut = cases.wide_table(64, nc)
    codes = cases.random_codes(cases.GATHER_ROWS, 64, nc)
    gcodes = mse.Codes(codes)
    want = opq.asymmetric_dot_product(lut, codes)
    for n_ids in cases.GATHER_COUNTS + [cases.second_trip_ids(n_cu())]:
        ids = cases.gather_ids(n_ids)
        assert np.array_equal(gpq.adc_gather(gcodes, lut, ids), want[ids]), n_ids


@pytest.mark.parametrize("n_chunks,nc,n_desc", [(64, 256, 0)] + cases.DESC_SHAPES)
def test_gathered_ids_past_the_end_give_the_minimum(gpu, mse, orc, n_chunks, nc, n_desc):
    opq, gpq = adc_pair(mse, orc, n_chunks, nc)
    lut = cases.wide_table(n_chunks, nc)
    codes = cases.random_codes(cases.GATHER_ROWS, n_chunks, nc)
    ids, bad = cases.bad_ids()
    if n_desc:
        desc, scales = cases.descriptors(cases.GATHER_ROWS, n_desc), cases.mixed_scales(n_desc)
        got = gpq.adc_gather(mse.Codes(codes, desc), lut, ids, scales)
        want = opq.adc_desc(lut, codes, desc, scales)
    else:
        got = gpq.adc_gather(mse.Codes(codes), lut, ids)
        want = opq.asymmetric_dot_product(lut, codes)
    assert np.all(got[bad] == I64_MIN)
    assert np.array_equal(got[~bad], want[ids[~bad]])


@pytest.mark.parametrize("n_chunks,nc,n_desc", cases.DESC_SHAPES)
def test_gathered_with_descriptors(gpu, mse, orc, n_chunks, nc, n_desc):
    """n_desc = 4 on 64 chunks stays on the fast path; 3 and 7 drop to the generic body and its descriptor loop; a 16-chunk codec takes
    the generic body with four.  Scales of both signs, descriptor bytes 0 and 255."""
    opq, gpq = adc_pair(mse, orc, n_chunks, nc)
    lut = cases.wide_table(n_chunks, nc)
    codes = cases.random_codes(cases.GATHER_ROWS, n_chunks, nc)
    desc, scales = cases.descriptors(cases.GATHER_ROWS, n_desc), cases.mixed_scales(n_desc)
    gcodes = mse.Codes(codes, desc)
    want = opq.adc_desc(lut, codes, desc, scales)
    plain = opq.asymmetric_dot_product(lut, codes)
    for n_ids in cases.GATHER_COUNTS:
        ids = cases.gather_ids(n_ids)
        assert np.array_equal(gpq.adc_gather(gcodes, lut, ids, scales), want[ids]), n_ids
    everyone = np.arange(cases.GATHER_ROWS, dtype=np.uint32)
    assert np.array_equal(gpq.adc_gather(gcodes, lut, everyone, scales), want)
    assert np.array_equal(gpq.adc_gather(gcodes, lut, everyone), plain)            # descriptors present, no scales: no bias


# ---- rank count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.RANK_ROWS)
def test_ranks_with_equal_scores_repeats_and_chunked_targets(gpu, mse, orc, n):
    base, query = cases.rank_base(orc, n)
    want = orc.ranks_from_scores(orc.score_all(base, query))
    s = mse.Searcher(mse.VectorList.from_f16s(base, cases.RANK_D))
    for m in cases.RANK_TARGETS:
        t = cases.rank_targets(n, m)
        assert np.array_equal(s.ranks(query, t), want[t]), m


# ---- f32 -> f16 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", [0, 1])
def test_index_add_rounds_half_to_even(gpu, mse, orc, part):
    """ScalarQuantizerIndex.add narrows f32 rows on the device.  48 rows of midpoints between neighbouring f16 values and their f32
    neighbours; a one-hot query reads one stored component back exactly, so labels and distances show every stored pattern."""
    f32_bits, want_bits = cases.f16_rounding_list()
    x = f32_bits.view(np.float32).reshape(2, 48, 64)[part]
    stored = want_bits.reshape(2, 48, 64)[part]
    assert np.array_equal(orc.f16_bits(x), stored)
    idx = mse.ScalarQuantizerIndex(64)
    idx.add(x)
    q = np.eye(64, dtype=np.float32)
    wd, wl = orc.index_search(stored, q, 48)
    res = idx.search(q, 48)                                   # more than 8 queries: the matrix-core pass and its exact re-score
    assert np.array_equal(res.labels, wl) and np.array_equal(res.distances, wd)
    for lo in range(0, 64, 8):                                # 8 at a time: the exact pass
        res = idx.search(q[lo:lo + 8], 48)
        assert np.array_equal(res.labels, wl[lo:lo + 8]) and np.array_equal(res.distances, wd[lo:lo + 8]), lo


def test_f32_queries_of_halfway_values_through_the_matrix_core_pass(gpu, mse, orc):
    """The same values as f32 QUERIES (narrowed on the device for the nomination scan) against the 64 one-hot rows."""
    f32_bits, _ = cases.f16_rounding_list()
    q = f32_bits.view(np.float32).reshape(96, 64)
    rows = np.eye(64, dtype=np.float32)
    idx = mse.ScalarQuantizerIndex(64)
    idx.add(rows)
    wd, wl = orc.index_search(orc.f16_bits(rows), q, 64)
    res = idx.search(q, 64)
    assert np.array_equal(res.labels, wl) and np.array_equal(res.distances, wd)


# ---- score model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SCORE_SHAPES)
def test_score_model_saturated_is_bit_exact(gpu, mse, orc, shape):
    """Every hidden pre-activation is >= 20 or <= -110: silu is the identity or -0 whatever expf's last bits are, and what is left are
    the two dot64 sums (lane l owns k = l mod 64, partial sums added in lane order), ragged in K and with idle waves in the last
    workgroup."""
    up, bias, down, x = cases.score_case(shape, saturated=True)
    got = mse.ScoreModel(up, bias, down).score_batch(x)
    want = orc.score_batch(up, bias, down, x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", cases.SCORE_SHAPES)
def test_score_model_unsaturated_within_the_stated_tolerance(gpu, mse, orc, shape):
    """Against float64, rtol = atol = 1e-5 (index_pack.hip's header) on outputs of order 1.
    Observed on an MI355X: the largest error is 0.026 of the tolerance (shape (100, 130, 2, 7)); the figure is printed per shape."""
    up, bias, down, x = cases.score_case(shape, saturated=False)
    got = mse.ScoreModel(up, bias, down).score_batch(x).astype(np.float64)
    want = cases.score_batch_f64(up, bias, down, x)
    ratio = float(np.max(np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want))))
    print("score model %s: largest error over tolerance %.4f" % (shape, ratio))
    assert ratio <= 1.0, ratio


# ---- descriptor buckets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdf_len", cases.BUCKET_CDF_LENS)
def test_descriptor_buckets(gpu, mse, orc, cdf_len):
    for n_desc, n in cases.BUCKET_SHAPES:
        cdfs = cases.bucket_cdfs(n_desc, cdf_len)
        scores = cases.bucket_scores(cdfs, n)
        assert np.array_equal(mse.descriptor_buckets(cdfs, scores), orc.descriptor_buckets(cdfs, scores)), (n_desc, n)
