"""Sparse-autoencoder features on the device (csrc/sae.hip, csrc/sae_api.hip) against tests/sae_ref.py's restatement of the rule, bit for
bit: the pre-activation chain of the f32 MFMA, relu, the exact selection streamed over d_hidden, the merge of the hidden parts, the
reconstruction and its squared error; and against float64 within bounds made from the operands.  tests/test_sae_host.py shows on the
CPU that the restatement is torch.kthvalue plus the strict mask of the reference's sae/model.py:32-41."""
import functools

import numpy as np
import pytest

import sae_ref as ref
from test_gpu_describe import gamma, U

pytestmark = pytest.mark.gpu

# The kernel's tile (csrc/sae.hip): 128 rows per workgroup, 128 hidden units per step, k in steps of 32; a thread loads 16 consecutive k,
# 16 bytes at a time where d_emb is a multiple of 8.  (d_emb, d_hidden, top_k, rows, bias): rows 1, one tile - 1 / whole / + 1, two tiles
# + 1; d_emb 1152 (vector loads), 72 (vector loads, ragged k step), 75 (guarded loads), 1; d_hidden 2, one tile + 1, two tiles, two
# tiles + 44, sixteen tiles; top_k 1, 128, 256 and d_hidden - 1 (three times).
SHAPES = [(1152, 2048, 128, 5, False), (1152, 300, 256, 257, True), (72, 129, 128, 127, True), (75, 256, 1, 128, False),
          (75, 300, 256, 129, True), (1, 2, 1, 129, True), (72, 256, 255, 1, False)]


@functools.lru_cache(maxsize=None)
def case(shape, seed=0):
    """(up, up_bias, down, down_bias, x as f16 bits, x widened to f32) -- random weights of a checkpoint's scale; with a bias, one that
    makes most units positive, so that the selection is among many"""
    d_emb, d_hidden, _, rows, bias = shape
    rng = np.random.default_rng(1000 + seed + d_emb + 7 * d_hidden)
    up = (rng.standard_normal((d_hidden, d_emb)) / np.sqrt(d_emb)).astype(np.float32)
    down = (rng.standard_normal((d_emb, d_hidden)) / np.sqrt(d_hidden)).astype(np.float32)
    up_bias = (rng.standard_normal(d_hidden) * 0.5 + 1.0).astype(np.float32) if bias else None
    down_bias = rng.standard_normal(d_emb).astype(np.float32) if bias else None
    xh = rng.standard_normal((rows, d_emb)).astype(np.float16)
    return up, up_bias, down, down_bias, xh.view(np.uint16), xh.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(shape, seed=0):
    """(counts, features, activations, reconstruction, squared errors) by the restatement; computed once per shape"""
    up, up_bias, down, down_bias, _, x = case(shape, seed)
    counts, feats, acts = ref.encode(up, x, shape[2], up_bias)
    recon = ref.reconstruct(down, down_bias, counts, feats, acts)
    out = (counts, feats, acts, recon, ref.sq_errors(recon, x))
    for a in out:
        a.setflags(write=False)
    return out


def model_of(mse, shape, seed=0):
    up, up_bias, down, down_bias, _, _ = case(shape, seed)
    return mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=shape[2])


def same_table(got, want):
    """got: a RowFeatures or a (counts, features, activations) triple; want: a triple"""
    g = got.to_host() if hasattr(got, "to_host") else got
    return (np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1])
            and np.array_equal(np.asarray(g[2]).view(np.uint32), np.asarray(want[2]).view(np.uint32)))


def encode_both_ways(mse, sae, xbits, **kw):
    """through the host-rows entry point and, when the width allows a base (a multiple of 64), through one: the same bytes"""
    got = sae.encode(xbits, **kw)
    if xbits.shape[1] % 64 == 0:
        assert same_table(sae.encode_rows(mse.VectorList.from_f16s(xbits, xbits.shape[1]), **kw), got.to_host())
    return got


# ---- the rule, shape by shape ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_features_reconstruction_and_error_are_the_restated_rule(gpu, mse, shape):
    _, _, _, _, xbits, _ = case(shape)
    counts, feats, acts, recon, sq = reference(shape)
    sae = model_of(mse, shape)
    got = encode_both_ways(mse, sae, xbits)
    assert len(got) == shape[3] and got.top_k == shape[2] and got.invalid_rows == 0
    assert same_table(got, (counts, feats, acts))
    assert counts.max() <= shape[2] and counts.min() >= 0
    assert np.array_equal(got.reconstruct().view(np.uint32), recon.view(np.uint32))
    assert np.array_equal(got.sq_errors().view(np.uint64), sq.view(np.uint64))
    assert got.mse() == float(sq.sum() / (shape[3] * shape[0]))


def test_hand_made_ties(gpu, mse):
    up, x, top_k, want = ref.tie_case()
    down = np.zeros((up.shape[1], up.shape[0]), np.float32)
    got = mse.SparseAutoencoder(up, down, top_k=top_k).encode(x.astype(np.float16))
    assert np.array_equal(got.counts, want), got.counts
    assert same_table(got, ref.encode(up, x, top_k))


@pytest.mark.parametrize("top_k", [1, 7, 128])
def test_small_integer_operands_tie_everywhere(gpu, mse, top_k):
    """weights and rows in -2 .. 2 over 8 components: a row's 300 activations take a handful of values"""
    rng = np.random.default_rng(top_k)
    up = rng.integers(-2, 3, (300, 8)).astype(np.float32)
    down = rng.integers(-2, 3, (8, 300)).astype(np.float32)
    x = rng.integers(-2, 3, (131, 8)).astype(np.float32)
    bias = rng.integers(-1, 2, 300).astype(np.float32)
    want = ref.encode(up, x, top_k, bias)
    assert (want[0] < top_k).any()                         # ties at the threshold cost features
    got = mse.SparseAutoencoder(up, down, bias, None, top_k=top_k).encode(x.astype(np.float16))
    assert same_table(got, want)
    assert np.array_equal(got.reconstruct().view(np.uint32), ref.reconstruct(down, None, *want).view(np.uint32))


# ---- candidate lists ----------------------------------------------------------------------------------------------------------------------
def ramp_case(d_hidden, rising):
    """d_emb 8; component 0 of up is a ramp over the features, so rows along e_0 see activations that rise (every value is a candidate
    and the list is cut as often as it can be) or fall (nothing passes after the first tile) with the feature index; component 1 is noise.
    The bias is positive: a unit past d_hidden in a ragged last tile would show up as a candidate."""
    rng = np.random.default_rng(d_hidden)
    up = np.zeros((d_hidden, 8), np.float32)
    ramp = (np.arange(d_hidden) + 1).astype(np.float32) / np.float32(8192)
    up[:, 0] = ramp if rising else ramp[::-1]
    up[:, 1] = rng.standard_normal(d_hidden).astype(np.float32)
    x = np.zeros((5, 8), np.float32)
    x[0, 0], x[1, 0], x[2, 0], x[3, 1], x[4, 0] = 1, 2, 0.5, 1.5, -1
    x[4, 1] = 0.25
    bias = np.full(d_hidden, 0.25, np.float32)
    return up, bias, x


@pytest.mark.parametrize("d_hidden", [4096, 4000])
@pytest.mark.parametrize("rising", [True, False])
def test_candidate_lists_that_always_and_never_grow(gpu, mse, d_hidden, rising):
    up, bias, x = ramp_case(d_hidden, rising)
    want = ref.encode(up, x, 128, bias)
    assert (want[0][:3] == 128).all()
    sae = mse.SparseAutoencoder(up, np.zeros((8, d_hidden), np.float32), bias, None, top_k=128)
    for parts in (1, 0, 5):
        sae.set_hidden_parts(parts)
        assert same_table(sae.encode(x.astype(np.float16)), want), parts


# ---- invariances ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1]])
def test_hidden_split_and_repetition_leave_the_bytes(gpu, mse, shape):
    _, _, _, _, xbits, _ = case(shape)
    want = reference(shape)[:3]
    sae = model_of(mse, shape)
    vecs = mse.VectorList.from_f16s(xbits, shape[0])
    for parts in (1, 2, 3, 0, 0, 1024):
        sae.set_hidden_parts(parts)
        assert same_table(sae.encode_rows(vecs), want), parts


def test_batch_invariance_is_bitwise(gpu, mse):
    """Row r through six calls: alone; the last row of a ragged call; inside a three-tile call; through ids in shuffled order with r
    repeated; from a first-offset range; from host rows."""
    shape = SHAPES[1]
    n, r = shape[3], 128 + 72
    _, _, _, _, xbits, _ = case(shape)
    want = reference(shape)[:3]
    sae = model_of(mse, shape)
    vecs = mse.VectorList.from_f16s(xbits, shape[0])
    one = tuple(a[r:r + 1] for a in want)
    assert same_table(sae.encode_rows(vecs), want)
    assert same_table(sae.encode_rows(vecs, ids=[r]), one)
    assert same_table(tuple(a[-1:] for a in sae.encode_rows(vecs, first=0, n=r + 1).to_host()), one)
    assert same_table(tuple(a[3:4] for a in sae.encode_rows(vecs, first=r - 3, n=10).to_host()), one)
    assert same_table(sae.encode(xbits[r:r + 1]), one)
    ids = np.random.default_rng(3).permutation(n)[:200].astype(np.uint32)
    ids[[0, 100, 199]] = r
    assert same_table(sae.encode_rows(mse.Searcher(vecs), ids=ids), tuple(a[ids] for a in want))
    assert same_table(sae.encode_rows(xbits, ids=ids), tuple(a[ids] for a in want))


# ---- invalid rows -------------------------------------------------------------------------------------------------------------------------
def test_nan_rows_are_flagged_and_their_neighbours_untouched(gpu, mse):
    rng = np.random.default_rng(11)
    d_emb, d_hidden, top_k, rows = 72, 300, 16, 130
    up = (rng.standard_normal((d_hidden, d_emb)) / 8).astype(np.float32)
    up[:, 5] = 0                                           # an inf at component 5 meets only zero weights: inf * 0
    up[:, 11] = -np.abs(up[:, 11]) - 1
    up[7, 11] = 0.5                                        # an inf at component 11 gives one +inf activation and 299 -inf
    down = (rng.standard_normal((d_emb, d_hidden)) / 16).astype(np.float32)
    xh = rng.standard_normal((rows, d_emb)).astype(np.float16)
    xh[3, 5] = np.inf
    xh[64, 9] = np.nan
    xh[129, 11] = np.inf
    want = ref.encode(up, xh.astype(np.float32), top_k)
    assert want[0][3] == ref.NONE and want[0][64] == ref.NONE and want[0][129] == 1
    sae = mse.SparseAutoencoder(up, down, top_k=top_k)
    for parts in (0, 1):
        sae.set_hidden_parts(parts)
        got = sae.encode(xh, count=True)
        assert got.invalid_rows == 2
        assert same_table(got, want)
        assert got.features[129, 0] == 7 and np.isposinf(got.activations[129, 0])
    valid = np.ones(rows, bool)
    valid[[3, 64]] = False
    assert np.array_equal(sae.counters(), 2 * ref.counters(*want[:2], d_hidden))
    sq = got.sq_errors()
    assert np.isnan(sq[~valid]).all() and np.isnan(got.reconstruct()[~valid]).all()
    finite = valid.copy()
    finite[129] = False                                    # the +inf activation's reconstruction is inf and NaN: no bits to compare
    recon = ref.reconstruct(down, None, *want)
    assert np.array_equal(got.reconstruct()[finite].view(np.uint32), recon[finite].view(np.uint32))
    assert np.array_equal(sq[finite].view(np.uint64), ref.sq_errors(recon, xh.astype(np.float32))[finite].view(np.uint64))


# ---- counters -------------------------------------------------------------------------------------------------------------------------------
def test_counters_accumulate_and_reset(gpu, mse):
    shape = SHAPES[4]
    _, _, _, _, xbits, _ = case(shape)
    counts, feats, _, _, _ = reference(shape)
    d_hidden = shape[1]
    once = ref.counters(counts, feats, d_hidden)
    flat = np.concatenate([feats[b, :counts[b]] for b in range(counts.size)]).astype(np.int64)
    assert np.array_equal(once, np.bincount(flat, minlength=d_hidden))
    sae = model_of(mse, shape)
    assert not sae.counters().any()
    sae.encode(xbits)
    assert np.array_equal(sae.counters(), once)
    sae.encode(xbits, count=False)
    assert np.array_equal(sae.counters(), once)
    sae.encode(xbits[:50])
    assert np.array_equal(sae.counters(reset=True), once + ref.counters(counts[:50], feats[:50], d_hidden))
    assert not sae.counters().any()


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[4]])
def test_reconstruction_within_the_bound_of_its_operands(gpu, mse, shape):
    """r_d is a chain of c = count fmas from down_bias[d]: c roundings, so |r^ - r| <= gamma_c (sum_i |a_i| |down[d][f_i]| + |down_bias[d]|)
    against float64 over the kept activations as the device reports them."""
    _, _, down, down_bias, xbits, _ = case(shape)
    got = model_of(mse, shape).encode(xbits)
    counts, feats, acts = got.to_host()
    recon = got.reconstruct().astype(np.float64)
    d64 = down.astype(np.float64)
    b64 = np.zeros(shape[0]) if down_bias is None else down_bias.astype(np.float64)
    worst = 0.0
    for b in range(shape[3]):
        f, a = feats[b, :counts[b]].astype(np.int64), acts[b, :counts[b]].astype(np.float64)
        want = d64[:, f] @ a + b64
        bound = gamma(int(counts[b])) * (np.abs(d64[:, f]) @ np.abs(a) + np.abs(b64))
        assert (np.abs(recon[b] - want) <= bound).all(), b
        worst = max(worst, float(np.max(np.abs(recon[b] - want) / np.maximum(bound, 1e-300))))
    print("sae reconstruction %s: largest observed / bound %.3g" % (shape, worst))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[4]])
def test_kept_set_against_float64(gpu, mse, shape):
    """z in float64, t64 its (top_k + 1)-th largest relu, B_j = gamma_{d_emb} sum_k |up[j][k]| |x_k| + u |z_j| the bound on the f32 chain
    and the bias add: every kept feature has z64_j >= t64 - 2 max B and every feature with z64_j > t64 + 2 max B is kept."""
    up, up_bias, _, _, xbits, x = case(shape)
    d_emb, d_hidden, top_k, rows, _ = shape
    counts, feats, _ = model_of(mse, shape).encode(xbits).to_host()
    up64, x64 = up.astype(np.float64), x.astype(np.float64)
    z = x64 @ up64.T + (0.0 if up_bias is None else up_bias.astype(np.float64)[None, :])
    B = gamma(d_emb) * (np.abs(x64) @ np.abs(up64).T) + U * np.abs(z)
    t = np.sort(np.maximum(z, 0.0), axis=1)[:, d_hidden - top_k - 1]
    slack = 2 * B.max(axis=1)
    for b in range(rows):
        kept = np.zeros(d_hidden, bool)
        kept[feats[b, :counts[b]].astype(np.int64)] = True
        assert (z[b][kept] >= t[b] - slack[b]).all(), b
        assert kept[z[b] > t[b] + slack[b]].all(), b


# ---- filters ------------------------------------------------------------------------------------------------------------------------------------
FILTER_SHAPE = (64, 300, 16, 500, True)


def mask_of(table, feature, min_activation, n_rows, rows_of):
    counts, feats, acts = table
    m = np.zeros(n_rows, bool)
    for i in range(counts.size):
        c = counts[i]
        if c != ref.NONE and ((feats[i, :c] == feature) & (acts[i, :c] >= min_activation)).any():
            m[rows_of[i]] = True
    return m


def test_feature_filter_is_the_mask_of_the_table(gpu, mse, orc):
    from test_gpu_filtered_graph import knn_graph
    from test_gpu_graph_delete import cfgs
    shape = FILTER_SHAPE
    n = shape[3]
    _, _, _, _, xbits, x = case(shape)
    sae = model_of(mse, shape)
    vecs = mse.VectorList.from_f16s(xbits, 64)
    searcher = mse.Searcher(vecs)
    whole = sae.encode_rows(vecs)
    counts, feats, acts = whole.to_host()
    kept = np.concatenate([feats[i, :counts[i]] for i in range(n)])
    feature = int(np.bincount(kept.astype(np.int64)).argmax())
    level = float(np.float32(np.median(acts[feats == feature])))
    want = mask_of((counts, feats, acts), feature, level, n, np.arange(n))
    assert 0 < want.sum() < (feats == feature).any(axis=1).sum()
    flt = whole.filter(feature, level)
    assert len(flt) == n and np.array_equal(flt.to_mask(), want)
    assert np.array_equal(whole.filter(feature).to_mask(), mask_of((counts, feats, acts), feature, 0.0, n, np.arange(n)))
    # a range at an offset and an id list with repeats speak of base rows; a table of host rows of its own rows
    part = sae.encode_rows(searcher, first=100, n=200)
    assert np.array_equal(part.filter(feature, level).to_mask(), mask_of(part.to_host(), feature, level, n, 100 + np.arange(200)))
    ids = np.random.default_rng(5).integers(0, n, 150).astype(np.uint32)
    ids[[3, 70]] = ids[0]
    g_adj, g_deg = knn_graph(x, 16, np.random.default_rng(6))
    g = mse.DeviceGraph(mse.IndexGraph(g_adj, g_deg), np.ones(n, np.uint8))
    by_ids = g.encode_features(sae, searcher, ids=ids)
    assert same_table(by_ids, (counts[ids], feats[ids], acts[ids]))
    assert np.array_equal(by_ids.filter(feature, level).to_mask(), mask_of(by_ids.to_host(), feature, level, n, ids))
    host = sae.encode(xbits[100:300])
    assert len(host.filter(feature, level)) == 200
    assert np.array_equal(host.filter(feature, level).to_mask(), want[100:300])
    # the filtered search equals the search over those rows alone
    queries = sae.feature_queries([feature, (feature + 1) % shape[1]])
    assert queries.shape == (2, 64) and queries.dtype == np.uint16
    k = 5
    assert flt.count >= k
    s1, i1 = searcher.bruteforce_topk(queries, k, mse.MODE_EXACT, allow=flt)
    s2, i2 = mse.Searcher(vecs.select(flt)).bruteforce_topk(queries, k, mse.MODE_EXACT)
    assert np.array_equal(s1, s2) and np.array_equal(i1, flt.ids()[i2])
    # ... and names rows to delete
    _, mcfg = cfgs(orc, mse, r=16, l=64, maxc=250)
    assert g.delete_rows(searcher, flt, mcfg)["deleted"] == flt.count
    g.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handles_usable(gpu, mse):
    shape = FILTER_SHAPE
    n = shape[3]
    up, up_bias, down, down_bias, xbits, _ = case(shape)
    want = tuple(a[:40] for a in ref.encode(up, case(shape)[5][:40], shape[2], up_bias))
    sae = model_of(mse, shape)
    vecs = mse.VectorList.from_f16s(xbits, 64)
    table = sae.encode_rows(vecs, n=40)
    assert same_table(table, want)
    wide = mse.VectorList.from_f16s(np.zeros((4, 128), np.uint16), 128)
    with pytest.raises(mse.MseError, match="d_emb is 64 .* 128"):
        sae.encode_rows(wide)
    with pytest.raises(mse.MseError, match="d_emb is 64 .* 72"):
        sae.encode(np.zeros((3, 72), np.uint16))
    with pytest.raises(mse.MseError, match="id 500 .* 500 rows"):
        sae.encode_rows(vecs, ids=[0, n])
    with pytest.raises(mse.MseError, match="not within"):
        sae.encode_rows(vecs, first=n - 5, n=6)
    for top_k in (0, 257, shape[1]):
        with pytest.raises(mse.MseError, match="top_k"):
            mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=top_k)
    host_rows = np.ascontiguousarray(xbits[:8])
    on_host = mse.VectorList.wrap_device(host_rows.ctypes.data, 8, 64, keepalive=host_rows)
    with pytest.raises(mse.MseError, match="not device memory"):
        sae.encode_rows(on_host)
    other = model_of(mse, shape)
    with pytest.raises(mse.MseError, match="another model"):
        table.reconstruct(model=other)
    with pytest.raises(mse.MseError, match="another model"):
        table.sq_errors(model=other)
    with pytest.raises(mse.MseError, match="row 39 .* 39 rows"):
        table.filter(0, n_rows=39)
    with pytest.raises(mse.MseError, match="feature 300"):
        table.filter(300)
    with pytest.raises(mse.MseError, match="parts"):
        sae.set_hidden_parts(1025)
    # the same handles, after all of that
    recon = ref.reconstruct(down, down_bias, *want)
    assert np.array_equal(table.reconstruct().view(np.uint32), recon.view(np.uint32))
    assert same_table(sae.encode_rows(vecs, n=40), want)
    assert same_table(other.encode_rows(vecs, n=40), want)
    assert len(table.filter(0, n_rows=40)) == 40


def test_a_checkpoint_state_dict_loads(gpu, mse):
    """up_proj / down_proj built as the reference's model.py:20-22 builds them, through from_state_dict"""
    import torch
    torch.manual_seed(3)
    d_emb, d_hidden, top_k = 72, 200, 9
    up_proj = torch.nn.Linear(d_emb, d_hidden, bias=False)
    down_proj = torch.nn.Linear(d_hidden, d_emb)
    down_proj.weight = torch.nn.Parameter(up_proj.weight.T.clone())
    sd = {"up_proj.weight": up_proj.weight, "down_proj.weight": down_proj.weight, "down_proj.bias": down_proj.bias}
    sae = mse.SparseAutoencoder.from_state_dict(sd, top_k)
    assert (sae.d_emb, sae.d_hidden, sae.top_k) == (d_emb, d_hidden, top_k)
    xh = np.random.default_rng(4).standard_normal((7, d_emb)).astype(np.float16)
    up, down, bias = up_proj.weight.detach().numpy(), down_proj.weight.detach().numpy(), down_proj.bias.detach().numpy()
    want = ref.encode(up, xh.astype(np.float32), top_k)
    got = sae.encode(xh)
    assert same_table(got, want)
    assert np.array_equal(got.reconstruct().view(np.uint32), ref.reconstruct(down, bias, *want).view(np.uint32))
