"""Descriptors on the device (csrc/describe.hip, csrc/describe_api.hip): the fused score MLP against tests/describe_ref.py's restatement
of its summation orders (bit for bit where silu is saturated) and against float64; the multi-rank radix select against numpy.sort; the
CDF fit against numpy.quantile; the descriptor bytes written into resident codes against the oracle's bucket search, alone and on a small
live index.  tests/test_describe_host.py shows on the CPU that the restatement is what it claims."""
import functools

import numpy as np
import pytest

import describe_ref as ref
import pq_codec_cases as cases
from conftest import make_pq
from test_describe_host import key_sets, ranks_for, f32_ties, timestamps

pytestmark = pytest.mark.gpu

# The kernel's tile (csrc/describe.hip): ROW_TILE = 128 rows per workgroup, HID_TILE = 128 hidden units per step in two halves of 64,
# K_STEP = 32.  (d_emb, d_hidden, out_ch, rows): rows on both sides of one tile and past two (1 is in SCORE_SHAPES); d_hidden 1, one
# hidden tile - 1 / + 1 and three tiles + 5 (in the last, one half of the last tile is empty and the other holds 5 units); d_emb 1, 33
# (one k step + 1), 63 and 65 (two k steps - 1 / + 1) and the product's 1152; 1, 3 and 8 output channels.
T, H, KS = ref.ROW_TILE, ref.HID_TILE, ref.K_STEP
TILE_SHAPES = [(63, H - 1, 1, T - 1), (65, H + 1, 3, T), (63, 3 * H + 5, 8, T + 1), (65, 1, 8, 2 * T + 3), (1, H, 3, 2 * T + 3),
               (KS + 1, H, 2, 5), (1152, H + 1, 3, T + 1)]
SHIPPED = (1152, 18432, 3, 130)         # meme-rater/ensemble_to_wide_model.py: 16 x 1152 hidden units, 3 outputs
U = 2.0 ** -24                          # unit roundoff of f32


def gamma(k):
    return k * U / (1 - k * U)


def f16_case(shape, saturated):
    """score_case with x rounded to f16: (up, bias, down, x as f16 bits, x widened back to f32 -- what both sides see)"""
    up, bias, down, x = cases.score_case(shape, saturated)
    xh = x.astype(np.float16)
    return up, bias, down, xh.view(np.uint16), xh.astype(np.float32)


def device_scores(mse, sm, xbits, **kw):
    """through a base when the width allows one (a multiple of 64), and through the host-rows entry point: the same kernel, the same bits"""
    got = sm.score_rows(xbits, **kw).to_host()
    if xbits.shape[1] % 64 == 0:
        via_base = sm.score_rows(mse.VectorList.from_f16s(xbits, xbits.shape[1]), **kw).to_host()
        assert np.array_equal(via_base.view(np.uint32), got.view(np.uint32))
    return got


# ---- the MLP --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SCORE_SHAPES + TILE_SHAPES)
def test_saturated_scores_are_the_restated_orders_bit_for_bit(gpu, mse, shape):
    """Every pre-activation is >= 20 or <= -110, so silu is the identity or -0 whatever expf's last bits are: what is compared is the
    k-ascending fma chain of the f32 MFMA, the bias add, and the hidden sum in the order the kernel's header states."""
    up, bias, down, xbits, x = f16_case(shape, saturated=True)
    got = device_scores(mse, mse.ScoreModel(up, bias, down), xbits)
    want = ref.score_rows(up, bias, down, x)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", cases.SCORE_SHAPES)
def test_unsaturated_scores_within_the_project_tolerance(gpu, mse, shape):
    """Against float64 on the f16-rounded rows, rtol = atol = 1e-5 (index_pack.hip's tolerance for the same model).
    Observed on an MI355X: the largest error is 0.047 of the tolerance (shape (100, 130, 2, 7)); the figure is printed per shape."""
    up, bias, down, xbits, x = f16_case(shape, saturated=False)
    got = device_scores(mse, mse.ScoreModel(up, bias, down), xbits).astype(np.float64)
    want = cases.score_batch_f64(up, bias, down, x)
    ratio = float(np.max(np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want))))
    print("fused score model %s: largest error over tolerance %.4f" % (shape, ratio))
    assert ratio <= 1.0, ratio


def shipped_bound(up, bias, down, x):
    """(float64 scores, bound), both [rows, out_ch]; the derivation is in the docstring of the test below."""
    d_emb, d_hidden = up.shape[1], up.shape[0]
    up64, x64, down64 = up.astype(np.float64), x.astype(np.float64), down.astype(np.float64)
    z = x64 @ up64.T + bias.astype(np.float64)[None, :]
    A = np.abs(x64) @ np.abs(up64).T
    e_s = gamma(d_emb) * A * (1 + U) + U * np.abs(z)
    h = z / (1.0 + np.exp(-z))
    e_h = 1.1 * e_s + gamma(4) * (np.abs(h) + 1.1 * e_s)
    depth = -(-d_hidden // H) + 10
    scale = d_emb / d_hidden
    bound = scale * ((1 + gamma(depth)) * (e_h @ np.abs(down64).T) + gamma(depth) * (np.abs(h) @ np.abs(down64).T))
    return h @ down64.T * scale, bound


def test_shipped_shape_within_the_bound_of_its_operands(gpu, mse):
    """(1152, 18 432, 3) over 130 rows (two row tiles, the second with two rows) against float64, within a bound B[b][c] made from the
    operands.  u = 2^-24, gamma_k = k u / (1 - k u); z = up . x + bias exactly, A[b][n] = sum_k |up[n][k]| |x[b][k]|.
      pre-activation  the MFMA is one k-ascending f32 fma chain of K = d_emb terms from 0 (the programming guide's FP32-input MFMA
                      section): |s^ - s| <= gamma_K A.  The bias add rounds once more: |z^ - z| <= e_s = gamma_K A (1 + u) + u |z|.
      silu            silu' lies in [-0.0998, 1.0998], so |silu(z^) - silu(z)| <= 1.1 e_s.  The device forms z^ / (1 + expf(-z^)): expf is
                      within 1 ulp = 2 u relative (ROCm device-library documentation, OCML "exp: 1 ulp" for f32), which moves the
                      denominator 1 + E by at most 2 u relative since E / (1 + E) < 1; the add and the correctly rounded division add u
                      each: |h^ - silu(z^)| <= gamma_4 |silu(z^)|.  Together e_h = 1.1 e_s + gamma_4 (|h| + 1.1 e_s).  (Where expf
                      overflows, below z = -88, silu is under 1e-36 in magnitude and the device's -0 is within that.)
      hidden sum      a term h_n down[c][n] passes at most D roundings on its way into the score: product and fma (2), five butterfly
                      rounds, one add per hidden tile (ceil(d_hidden / 128) = 144), the add of the two halves, the scale's own rounding
                      and the multiplication by it (3): D = 144 + 10 -- the gamma_H of a sum whose depth is D rather than H because
                      the order is a tree across each tile.  |score^ - score| <= scale ((1 + gamma_D) sum_n |down| e_h + gamma_D sum_n |down| |h|).
    Observed on an MI355X: the largest observed / bound is 7.6e-06 (largest error 1.3e-06 on outputs up to 2.5): the bound is the
    worst case of 1152-term chains, the errors behave as a random walk.  The ratio is printed."""
    up, bias, down, xbits, x = f16_case(SHIPPED, saturated=False)
    got = mse.ScoreModel(up, bias, down).score_rows(mse.VectorList.from_f16s(xbits, SHIPPED[0])).to_host().astype(np.float64)
    want, bound = shipped_bound(up, bias, down, x)
    ratio = float(np.max(np.abs(got - want) / bound))
    print("fused score model %s: largest observed / bound %.3g (largest error %.3g, outputs up to %.3g)"
          % (SHIPPED, ratio, np.max(np.abs(got - want)), np.max(np.abs(want))))
    assert ratio <= 1.0, ratio


def test_batch_invariance_is_bitwise(gpu, mse):
    """Row r's scores through five calls: alone; the last row of a ragged call; in the middle of a three-tile call; through ids in
    shuffled order with r repeated; from a first-offset range.  Unsaturated, so expf's bits are in play too."""
    n, r = 3 * T + 5, T + 72
    up, bias, down, xbits, _ = f16_case((1152, 130, 3, n), saturated=False)
    sm = mse.ScoreModel(up, bias, down)
    vecs = mse.VectorList.from_f16s(xbits, 1152)
    whole = sm.score_rows(vecs).to_host()
    assert whole.shape == (n, 3)
    want = whole[r].view(np.uint32)
    assert np.array_equal(sm.score_rows(vecs, ids=[r]).to_host()[0].view(np.uint32), want)
    assert np.array_equal(sm.score_rows(vecs, first=0, n=r + 1).to_host()[-1].view(np.uint32), want)
    assert np.array_equal(sm.score_rows(vecs, first=r - 3, n=10).to_host()[3].view(np.uint32), want)
    ids = np.random.default_rng(3).permutation(n)[:300].astype(np.uint32)
    ids[[0, 150, 299]] = r
    by_ids = sm.score_rows(mse.Searcher(vecs), ids=ids).to_host()
    assert np.array_equal(by_ids.view(np.uint32), whole[ids].view(np.uint32))      # every row, wherever it stands


def test_one_handle_serves_the_old_and_the_new_path(gpu, mse, orc):
    shape = (100, 130, 2, 7)
    up, bias, down, xbits, x = f16_case(shape, saturated=True)
    sm = mse.ScoreModel(up, bias, down)
    old_want, new_want = orc.score_batch(up, bias, down, x), ref.score_rows(up, bias, down, x)
    for _ in range(2):
        assert np.array_equal(sm.score_batch(x).view(np.uint32), old_want.view(np.uint32))
        assert np.array_equal(sm.score_rows(xbits).to_host().view(np.uint32), new_want.view(np.uint32))


def test_mlp_errors_leave_the_handle_usable(gpu, mse):
    up, bias, down, xbits, x = f16_case((64, 65, 3, 9), saturated=True)
    sm = mse.ScoreModel(up, bias, down)
    vecs = mse.VectorList.from_f16s(xbits, 64)
    want = ref.score_rows(up, bias, down, x)
    wide = mse.VectorList.from_f16s(np.zeros((4, 128), np.uint16), 128)
    with pytest.raises(mse.MseError, match="d_emb is 64 .* 128"):
        sm.score_rows(wide)
    with pytest.raises(mse.MseError, match="id 9 .* 9 rows"):
        sm.score_rows(vecs, ids=[0, 9])
    with pytest.raises(mse.MseError, match="not within"):
        sm.score_rows(vecs, first=5, n=5)
    up9, bias9, down9, xb9, _ = f16_case((64, 65, 9, 2), saturated=True)
    nine = mse.ScoreModel(up9, bias9, down9)
    with pytest.raises(mse.MseError, match="9 output channels"):
        nine.score_rows(xb9)
    assert nine.score_batch(np.zeros((1, 64), np.float32)).shape == (1, 9)
    assert np.array_equal(sm.score_rows(vecs).to_host().view(np.uint32), want.view(np.uint32))


# ---- select and fit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 70001])
def test_order_statistics_are_the_sorted_order(gpu, mse, n):
    """Every key set of the host test, as channel 1 of a two-channel table (a strided column) or as the timestamp channel; all n
    ranks up to 512 keys, else the 255-quantile rank pairs, duplicates included."""
    r = ranks_for(n)
    other = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    for name, x in key_sets(n).items():
        if x.dtype == np.uint32:
            got = mse.RowScores.from_host(other[:, None], timestamps=x.astype(np.int64)).order_statistics(1, r)
        else:
            got = mse.RowScores.from_host(np.stack([other, x], axis=1)).order_statistics(1, r)
        want = np.sort(x)[r.astype(np.int64)]
        assert got.dtype == want.dtype and np.array_equal(got, want), name


def test_more_ranks_than_one_select_takes(gpu, mse):
    x = key_sets(70001)["normals"]
    r = np.random.default_rng(9).integers(0, x.size, 1300).astype(np.uint64)
    assert np.array_equal(mse.RowScores.from_host(x[:, None]).order_statistics(0, r), np.sort(x)[r.astype(np.int64)])


@pytest.mark.parametrize("n", [1, 2, 255, 70001])
def test_fit_is_numpy_quantile_narrowed_to_f32(gpu, mse, n):
    s = np.stack([key_sets(n)["normals"], f32_ties(n), key_sets(n)["last 10 bits"]], axis=1)
    ts = timestamps(n)
    rs = mse.RowScores.from_host(s, timestamps=ts)
    for cdf_len in (255, 3, 1):
        got = rs.fit_cdfs(cdf_len)
        want = np.stack([np.quantile(c, np.linspace(0, 1, cdf_len)) for c in (s[:, 0], s[:, 1], s[:, 2], ts)]).astype(np.float32)
        assert got.shape == (4, cdf_len) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), cdf_len
        assert np.array_equal(got.view(np.uint32), ref.fit_cdfs(s, ts, cdf_len).view(np.uint32))


def test_select_refusals(gpu, mse):
    x = key_sets(70001)["normals"].copy()
    x[12345] = np.nan
    rs = mse.RowScores.from_host(x[:, None])
    with pytest.raises(mse.MseError, match="1 NaN among the 70001 keys"):
        rs.order_statistics(0, [0])
    with pytest.raises(mse.MseError, match="NaN"):
        rs.fit_cdfs()
    with pytest.raises(mse.MseError, match="rank 70001"):
        mse.RowScores.from_host(x[:, None]).order_statistics(0, [70001])
    for bad in (-1, 2**32):
        with pytest.raises(mse.MseError, match=r"outside \[0, 2\^32\)"):
            mse.RowScores.from_host(np.zeros((3, 1), np.float32), timestamps=[5, bad, 7])
    with pytest.raises(mse.MseError, match="1 .. 255"):
        mse.RowScores.from_host(np.zeros((3, 1), np.float32)).fit_cdfs(256)


def test_select_is_deterministic(gpu, mse):
    s = np.stack([key_sets(70001)["normals"], f32_ties(70001)], axis=1)
    ts = timestamps(70001)
    runs = []
    for _ in range(2):
        rs = mse.RowScores.from_host(s, timestamps=ts)
        runs.append((rs.fit_cdfs().tobytes(), rs.order_statistics(1, ranks_for(70001)).tobytes(), rs.order_statistics(2, ranks_for(70001)).tobytes()))
    assert runs[0] == runs[1]


# ---- describe -----------------------------------------------------------------------------------------------------------------------------
N, D = 3000, 1152
SCALES = np.array([0.5, -0.25, 1.0, 0.125], np.float32) / np.float32(512)


@functools.lru_cache(maxsize=None)
def world_rows(orc):
    from test_gpu_filtered_graph import clustered_rows
    x = clustered_rows(orc, N + 200, D, n_centres=48, seed=91)
    ts = np.random.default_rng(92).integers(2**31 - 10**7, 2**31 + 10**7, N + 200).astype(np.int64)
    return x, orc.f16_bits(x), ts


@pytest.fixture(scope="module")
def model(gpu, mse):
    up, bias, down, _ = cases.score_case((D, 130, 3, 1), saturated=False)
    return mse.ScoreModel(up, bias, down)


def reference_bytes(orc, cdfs, scores, ts):
    return orc.descriptor_buckets(cdfs, np.concatenate([scores, np.asarray(ts).astype(np.float32)[:, None]], axis=1))


def test_fit_and_describe_resident_rows(gpu, mse, orc, model):
    """scores of 3 000 resident rows + timestamps -> fitted CDFs (== numpy.quantile of the downloaded scores) -> descriptor bytes in
    resident codes == the oracle's bucket search over the downloaded scores, byte for byte; the PQ codes are untouched."""
    _, bits, ts = world_rows(orc)
    vecs = mse.VectorList.from_f16s(bits[:N], D)
    rs = model.score_rows(vecs, timestamps=ts[:N])
    scores, ts_back = rs.to_host()
    assert np.array_equal(ts_back, ts[:N].astype(np.uint32)) and rs.n_desc == 4 and len(rs) == N
    cdfs = rs.fit_cdfs()
    want_cdfs = np.stack([np.quantile(c, np.linspace(0, 1, 255)) for c in (scores[:, 0], scores[:, 1], scores[:, 2], ts[:N])]).astype(np.float32)
    assert np.array_equal(cdfs.view(np.uint32), want_cdfs.view(np.uint32))
    pq_codes = np.random.default_rng(93).integers(0, 256, (N, 64), dtype=np.uint8)
    codes = mse.Codes(pq_codes, np.full((N, 4), 77, np.uint8))
    codes.describe(rs, cdfs)
    got_codes, got = codes.read_rows(0, N, descriptors=True)
    want = reference_bytes(orc, cdfs, scores, ts[:N])
    assert np.array_equal(got, want) and np.array_equal(got_codes, pq_codes)
    assert len(np.unique(want[:, 0])) > 200 and len(np.unique(want[:, 3])) > 200      # the fitted CDFs spread the rows over the buckets


@pytest.mark.parametrize("cdf_len", [1, 3, 255])
def test_describe_is_the_oracles_bucket_search(gpu, mse, orc, cdf_len):
    """CDFs with runs of equal entries and scores on, between and beyond their entries (+-inf, NaN and -0.0 among them)."""
    cdfs = cases.bucket_cdfs(4, cdf_len)
    scores = cases.bucket_scores(cdfs, N)[:, :3]
    ts = np.random.default_rng(94).integers(0, 2**32, N).astype(np.int64)
    cdfs[3] = np.sort(np.random.default_rng(95).choice(ts, cdf_len).astype(np.float32))   # the timestamp's CDF: f32-rounded timestamps
    rs = mse.RowScores.from_host(scores, timestamps=ts)
    codes = mse.Codes(np.zeros((N, 8), np.uint8), np.zeros((N, 4), np.uint8))
    codes.describe(rs, cdfs)
    assert np.array_equal(codes.read_rows(0, N, descriptors=True)[1], reference_bytes(orc, cdfs, scores, ts))


def test_describe_an_id_list_changes_only_those_rows(gpu, mse, orc, model):
    _, bits, ts = world_rows(orc)
    vecs = mse.VectorList.from_f16s(bits[:N], D)
    rng = np.random.default_rng(96)
    ids = rng.permutation(N)[:257].astype(np.uint32)
    rs = model.score_rows(vecs, ids=ids, timestamps=ts[ids])
    scores, _ = rs.to_host()
    cdfs = model.score_rows(vecs, timestamps=ts[:N]).fit_cdfs()
    pq_codes = rng.integers(0, 256, (N, 64), dtype=np.uint8)
    before = rng.integers(0, 256, (N, 4), dtype=np.uint8)
    codes = mse.Codes(pq_codes, before)
    codes.describe(rs, cdfs, ids=ids)
    want = before.copy()
    want[ids] = reference_bytes(orc, cdfs, scores, ts[ids])
    got_codes, got = codes.read_rows(0, N, descriptors=True)
    assert np.array_equal(got, want) and np.array_equal(got_codes, pq_codes)
    assert (want[ids] != before[ids]).any()
    # a range at an offset: rows 100 .. 356 take the same 257 entries
    codes2 = mse.Codes(pq_codes, before)
    codes2.describe(rs, cdfs, first=100)
    want2 = before.copy()
    want2[100:357] = want[ids]
    assert np.array_equal(codes2.read_rows(0, N, descriptors=True)[1], want2)
    # refusals leave the bytes as they were
    three = mse.Codes(pq_codes, before[:, :3])
    with pytest.raises(mse.MseError, match="3 descriptor bytes .* 4 channels"):
        three.describe(rs, cdfs, ids=ids)
    lib_three = mse.Codes(pq_codes, before[:, :3])
    with pytest.raises(mse.MseError, match="carry 3 descriptor bytes per row but the scores have 4 channels"):
        from mse import ffi
        import ctypes as C
        ffi.check(ffi.lib().mse_codes_describe(lib_three._h, None, rs._h, None, 0, cdfs.ctypes.data_as(C.POINTER(C.c_float)), 255), "codes_describe")
    assert np.array_equal(three.read_rows(0, N, descriptors=True)[1], before[:, :3])
    assert np.array_equal(lib_three.read_rows(0, N, descriptors=True)[1], before[:, :3])
    with pytest.raises(mse.MseError, match="id 3000"):
        codes.describe(rs, cdfs, ids=np.r_[ids[:256], N])
    with pytest.raises(mse.MseError, match="not within"):
        codes.describe(rs, cdfs, first=N - 100)
    assert np.array_equal(codes.read_rows(0, N, descriptors=True)[1], want)


def test_describe_inserted_rows_of_a_live_index(gpu, mse, orc, model):
    """A graph over the 3 000 rows with described codes; 200 rows deleted and 200 new ones inserted with zero descriptor bytes;
    DeviceGraph.describe for the inserted slots.  The descriptor filter then equals the numpy mask over the reference bytes, and an
    ADC-scored request with descriptor scales answers as a fresh upload of codes carrying the reference bytes does."""
    from test_gpu_filtered_graph import knn_graph
    from test_gpu_graph_delete import cfgs
    x, bits, ts = world_rows(orc)
    rng = np.random.default_rng(97)
    cents, Tm, _, _ = make_pq(orc)
    gpq = mse.ProductQuantizer(cents, Tm, 18, D)
    vecs = mse.VectorList.from_f16s(bits[:N], D)
    searcher = mse.Searcher(vecs)
    rs = model.score_rows(vecs, timestamps=ts[:N])
    cdfs = rs.fit_cdfs()
    codes = mse.Codes.quantize_base(gpq, vecs, np.zeros((N, 4), np.uint8))
    codes.describe(rs, cdfs)
    adj, degs = knn_graph(x[:N], 16, rng)
    g = mse.DeviceGraph(mse.IndexGraph(adj, degs), np.ones(N, np.uint8))
    start = 7
    slots = rng.choice(np.setdiff1d(np.arange(N), [start]), 200, replace=False).astype(np.uint32)
    _, mcfg = cfgs(orc, mse, r=16, l=64, maxc=250)
    assert g.delete_rows(searcher, slots, mcfg)["deleted"] == 200
    fresh, fresh_ts = bits[N:], ts[N:]
    st = g.insert_rows(searcher, slots, fresh, mcfg, start, quantizer=gpq, codes=codes, descriptors=np.zeros((200, 4), np.uint8), batch=64)
    assert st["inserted"] == 200 and not codes.read_rows(0, N, descriptors=True)[1][slots].any()
    g.describe(codes, model.score_rows(searcher, ids=slots, timestamps=fresh_ts), cdfs, ids=slots)
    # the reference bytes: the oracle's buckets of the downloaded scores of the index as it is now
    rows2, ts2 = bits[:N].copy(), ts[:N].copy()
    rows2[slots], ts2[slots] = fresh, fresh_ts
    assert np.array_equal(vecs.rows(0, N), rows2)
    scores2, _ = model.score_rows(vecs, timestamps=ts2).to_host()
    want = reference_bytes(orc, cdfs, scores2, ts2)
    got_codes, got = codes.read_rows(0, N, descriptors=True)
    assert np.array_equal(got, want) and want[slots].any()
    ranges = {0: (10, 200), 3: (0, 128)}
    mask = (want[:, 0] >= 10) & (want[:, 0] <= 200) & (want[:, 3] <= 128)
    assert np.array_equal(mse.RowFilter.from_descriptors(codes, ranges).to_mask(), mask) and 0 < mask.sum() < N
    # one ADC-scored request with descriptor scales against a fresh upload
    h = g.to_host()
    vecs2 = mse.VectorList.from_f16s(rows2, D)
    twin_codes, twin_g = mse.Codes(got_codes, want), mse.DeviceGraph(mse.IndexGraph(h.adj, h.deg), np.ones(N, np.uint8))
    qs = orc.f16_to_f32(fresh[:6])
    starts = np.full(6, start, np.uint32)
    ids, sc, _ = mse.disk_query_topk(searcher, gpq, codes, g, qs, 10, starts, None, SCALES, False, 2, 64)
    wids, wsc, _ = mse.disk_query_topk(mse.Searcher(vecs2), gpq, twin_codes, twin_g, qs, 10, starts, None, SCALES, False, 2, 64)
    assert np.array_equal(ids, wids) and np.array_equal(sc, wsc)
    plain, psc, _ = mse.disk_query_topk(searcher, gpq, codes, g, qs, 10, starts, None, None, False, 2, 64)
    assert not np.array_equal(sc, psc)                                   # the descriptor bytes are in the scores
    g.close()
    twin_g.close()
