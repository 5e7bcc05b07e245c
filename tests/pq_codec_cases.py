"""Case builders for the codec and index-packing kernels (csrc/pq.hip, csrc/index_pack.hip) at the sizes where each of their code
paths begins or ends.  numpy only: tests/test_pq_codec_cases_host.py shows with the oracle alone that every case is what its comment
says, tests/test_gpu_pq_codec_edges.py holds the device to the oracle on the same cases."""
import functools

import numpy as np

from conftest import make_pq

I64_MIN = np.iinfo(np.int64).min


# ---- transform ----------------------------------------------------------------------------------------------------------------------
# (d, dpc): 18 = one chunk, below every tile; 72 = 64 + 8 (the vector kernel's 8-loop once, no scalar tail); 90 = 64 + 3 * 8 + 2 (all three
# loops; ragged in the 16-, 32- and 64-wide tiles); 144; 1152 (the product's width)
TRANSFORM_SHAPES = [(18, 18), (72, 8), (90, 5), (144, 18), (1152, 18)]
# both sides of the n >= 256 switch between the two batch kernels, ragged tiles in i, j and k on each side
TRANSFORM_BATCHES = [1, 15, 16, 17, 255, 256, 257, 320]


def skewed_codec(orc, d, dpc, n_centroids, seed=7):
    """make_pq's codec with its orthonormal matrix times a diagonal of magnitudes 2^-3 .. 2^3: neither orthonormal nor symmetric, so a
    transposed or mis-strided read of the matrix moves the result far more than rounding does."""
    cents, T, _, _ = make_pq(orc, d, dpc, n_centroids, seed)
    scale = np.exp2(np.random.default_rng(seed + 1000).uniform(-3.0, 3.0, d))
    return cents, np.ascontiguousarray((T.astype(np.float64) * scale[None, :]).astype(np.float32))


def transform_inputs(d, n=max(TRANSFORM_BATCHES), seed=11):
    return (np.random.default_rng(seed + d).standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _transform_case(orc, d, dpc):
    cents, T = skewed_codec(orc, d, dpc, 16)
    x = transform_inputs(d)
    opq = orc.PQ(cents, T, dpc, d)
    want = opq.apply_transform(x)
    want.setflags(write=False)
    return {"d": d, "dpc": dpc, "cents": cents, "T": T, "x": x, "want": want, "opq": opq}


def transform_case(orc, d, dpc):
    """The codec, the 320 input rows and the oracle's transform of all of them (rows are independent: a batch of n is want[:n])."""
    return _transform_case(orc, d, dpc)


# ---- quantise -----------------------------------------------------------------------------------------------------------------------
# dpc = 18 is the register-tiled kernel: one workgroup owns 256 x 4 vectors of one chunk and clamps vectors past n to row n - 1
TILED_WIDTHS = [18, 90, 1152]
TILED_CENTROIDS = [1, 3, 255, 256]
TILED_BATCHES = [1, 3, 4, 5, 1023, 1024, 1025, 2049]
TILED_BATCHES_1152 = [1, 1025]
GENERIC_SHAPES = [(64, 16), (72, 8), (90, 5)]
GENERIC_CENTROIDS = [4, 256]
GENERIC_BATCHES = [1, 257]


def tiled_batches(d):
    return TILED_BATCHES_1152 if d == 1152 else TILED_BATCHES


@functools.lru_cache(maxsize=None)
def _quantize_inputs(orc, d, n_max):
    """Input rows and the oracle's transform of them: make_pq draws its matrix before its centroids, so it is the same matrix for every
    centroid count and the transformed rows are shared."""
    _, T = skewed_codec(orc, d, d, 1, seed=21)
    x = transform_inputs(d, n_max, seed=23)
    return T, x, orc.PQ(np.zeros((1, d), np.float32), T, d, d).apply_transform(x)


@functools.lru_cache(maxsize=None)
def _quantize_case(orc, d, dpc, n_centroids, n_max):
    cents, T = skewed_codec(orc, d, dpc, n_centroids, seed=21)
    T0, x, t = _quantize_inputs(orc, d, n_max)
    assert np.array_equal(T, T0)
    want = orc.PQ(cents, T, dpc, d).quantize_batch(t, pre_transformed=True)
    want.setflags(write=False)
    return {"d": d, "dpc": dpc, "cents": cents, "T": T, "x": x, "want": want}


def quantize_case(orc, d, dpc, n_centroids, n_max):
    """Codec, n_max input rows and the oracle's codes of all of them (a batch of n is want[:n])."""
    return _quantize_case(orc, d, dpc, n_centroids, n_max)


def planted_tie_case(d, dpc, with_inf=False):
    """Small integers under the identity transform, so every product is exact.  Per chunk the centroids' sub-vectors are
        0: e0      1: 2 e1      2: 2 e2      3: 2 e1 (= 1)      4: 2 e2 (= 2)      5: 2 e2 (= 2)
    and the rows, chunk by chunk,
        row 0: e1    -> centroids 1 and 3 tie for the maximum                      -> 1, the lowest index
        row 1: e2    -> centroids 2, 4 and 5 tie                                   -> 2
        row 2: 0     -> every product is zero, 0 > -inf fires once, at centroid 0  -> 0
        row 3: e1 with chunk 1 set to NaN: the transform's 0 * NaN spreads it to every component, no `>` ever fires -> 0 everywhere
        rows 4 ..: copies of rows 0 and 1, so that the batch is no multiple of the tiled kernel's four vectors per thread
    with_inf: centroid 0's sub-vector of chunk 1 is -inf and every row is strictly positive, (1, 2, 1, 1, ...) per chunk: centroid 0 scores
    -inf there, which never beats the initial -inf, and 1 and 3 tie at 4 -> 1 in every chunk."""
    n_chunks = d // dpc
    cents = np.zeros((6, d), np.float32)
    for c in range(n_chunks):
        o = c * dpc
        cents[0, o] = 1.0
        cents[[1, 3], o + 1] = 2.0
        cents[[2, 4, 5], o + 2] = 2.0
    T = np.eye(d, dtype=np.float32)
    if with_inf:
        cents[0, dpc:2 * dpc] = -np.inf
        row = np.ones(d, np.float32)
        row[1::dpc] = 2.0
        x = np.tile(row, (5, 1))
        want = np.ones((5, n_chunks), np.uint8)
        return cents, T, x, want
    x = np.zeros((7, d), np.float32)
    x[0, 1::dpc] = 1.0
    x[1, 2::dpc] = 1.0
    x[3] = x[0]
    x[3, dpc:2 * dpc] = np.nan
    x[4], x[5], x[6] = x[1], x[0], x[1]
    want = np.zeros((7, n_chunks), np.uint8)
    want[[0, 5]] = 1
    want[[1, 4, 6]] = 2
    return cents, T, x, want


# widths that a VectorList can hold (multiples of 64): the generic kernel, and the tiled one at 32 chunks of 18
QUANTIZE_BASE_SHAPES = [(64, 16, 256), (576, 18, 256)]


def f16_edge_rows(orc, d, n=300, seed=31):
    """f16 rows (bit patterns) of data-like noise with f16 subnormals of both signs and +-65504 components sprinkled in."""
    rng = np.random.default_rng(seed + d)
    rows = orc.f16_bits((rng.standard_normal((n, d)) / np.sqrt(d)).astype(np.float32)).reshape(-1)
    where = rng.permutation(rows.size)
    k = rows.size // 20
    rows[where[:k]] = rng.integers(1, 0x400, k).astype(np.uint16) | (rng.integers(0, 2, k).astype(np.uint16) << 15)
    rows[where[k:k + 40]] = 0x7BFF
    rows[where[k + 40:k + 80]] = 0xFBFF
    return rows.reshape(n, d)


# ---- ADC ----------------------------------------------------------------------------------------------------------------------------
def adc_codec(n_chunks, n_centroids):
    """A codec of the given table shape (dpc = 1 keeps it small); the ADC calls use neither its centroids nor its transform."""
    return np.zeros((n_centroids, n_chunks), np.float32), np.eye(n_chunks, dtype=np.float32), 1, n_chunks


def wide_table(n_chunks, n_centroids, seed=41):
    """Entries of both signs, magnitudes 2^-20 .. 2^3: the order of the f32 adds shows in the result."""
    rng = np.random.default_rng(seed + 1000 * n_chunks + n_centroids)
    t = np.exp2(rng.uniform(-20.0, 3.0, (n_chunks, n_centroids))) * rng.choice([-1.0, 1.0], (n_chunks, n_centroids))
    return t.astype(np.float32)


def random_codes(n, n_chunks, n_centroids, seed=43):
    return np.random.default_rng(seed + n_chunks + n_centroids).integers(0, n_centroids, (n, n_chunks), dtype=np.uint8)


def reversed_sums(opq, lut, codes):
    """The same entries added in descending chunk order (through the oracle: reverse the table's rows and the codes' columns)."""
    return opq.asymmetric_dot_product(np.ascontiguousarray(lut[::-1]), np.ascontiguousarray(codes[:, ::-1]))


FRESH_SCAN_BATCHES = [65, 1, 63, 64, 127]          # 65 first: the fresh handle whose first call is a 64 x 256 scan with a partial last group
FULL_SCAN_CHUNKS = [16, 32, 5, 18]                 # 16-byte body (16, 32), byte body (5, 18)
FULL_SCAN_CENTROIDS = [3, 256]                     # chunks x 3 is no multiple of 4 at 5 chunks (scalar table copy); x 256 always is
FULL_SCAN_BATCHES = [1, 255, 256, 1023, 1024, 1025]   # workgroups of 256 and of 1024 threads, a ragged last one
GATHER_CENTROIDS = [256, 16]
GATHER_COUNTS = [1, 3, 4, 5, 4095, 4097]
GATHER_ROWS = 1000


def second_group_rows(n_cu):
    """One workgroup per CU, 16 waves each, a group of 64 rows per wave and trip: 65 rows more give one wave a full second group and
    another a ragged one."""
    return 64 * 16 * n_cu + 65


def second_trip_ids(n_cu):
    """At most 2 * CUs workgroups of 1024 threads, four ids per thread and trip: every thread makes a second trip, the last one ragged."""
    return 2 * n_cu * 4096 + 5


def gather_ids(n_ids, n_rows=GATHER_ROWS, seed=47):
    ids = np.random.default_rng(seed + n_ids).integers(0, n_rows, n_ids).astype(np.uint32)
    ids[0] = n_rows - 1
    if n_ids > 2:
        ids[1] = ids[2] = 0                        # a repeat
    return ids


def bad_ids(n_rows=GATHER_ROWS, n_ids=517, seed=53):
    """Valid ids with repeats, and at every 7th position an id past the end: len(codes) and 0xFFFFFFFF in turn."""
    ids = gather_ids(n_ids, n_rows, seed)
    bad = np.zeros(n_ids, bool)
    bad[3::7] = True
    ids[bad] = np.where(np.arange(bad.sum()) % 2 == 0, n_rows, 0xFFFFFFFF).astype(np.uint32)
    return ids, bad


def descriptors(n, n_desc, seed=59):
    d = np.random.default_rng(seed + n_desc).integers(0, 256, (n, n_desc), dtype=np.uint8)
    d[0], d[-1] = 0, 255
    d[1, ::2], d[1, 1::2] = 255, 0
    return d


def mixed_scales(n_desc):
    return (np.array([0.5, -0.25, 3.0, -1e-3, 0.125, -2.0, 0.75], np.float32)[:n_desc] / np.float32(512)).astype(np.float32)


# (n_chunks, n_centroids, n_desc): the gathered fast path; the generic body's descriptor loop on the same 64-chunk codec; another codec
DESC_SHAPES = [(64, 256, 4), (64, 256, 3), (64, 256, 7), (16, 256, 4)]


# ---- rank count ---------------------------------------------------------------------------------------------------------------------
RANK_D = 64
RANK_ROWS = [1, 63, 65, 1000]
RANK_TARGETS = [1, 1024, 1025, 2049]               # RANK_MAX_TARGETS = 1024 per launch: the host loop chunks from 1025 on


def rank_base(orc, n, seed=61):
    """n f16 rows of which only the first max(1, n // 3) are distinct: every other row is an exact copy of one of them, so most scores
    occur more than once and the (score desc, id asc) tie rule decides."""
    rng = np.random.default_rng(seed + n)
    m = max(1, n // 3)
    distinct = orc.f16_bits((rng.standard_normal((m, RANK_D)) / np.sqrt(RANK_D)).astype(np.float32))
    source = np.concatenate([np.arange(m), rng.integers(0, m, n - m)])
    source[m:m + 1] = 0                            # row 0 has a copy further down
    query = orc.f16_bits((rng.standard_normal(RANK_D) / np.sqrt(RANK_D)).astype(np.float32))
    return np.ascontiguousarray(distinct[source]), query


def rank_targets(n, m, seed=67):
    """m target rows: row 0, row n - 1, five repeats of one id, the rest drawn from all rows (two thirds of which are copies); a single
    target is row n - 1, a copy."""
    t = np.random.default_rng(seed + n + m).integers(0, n, m).astype(np.uint32)
    if m < 7:
        t[:] = n - 1
        return t
    for i, v in enumerate([0, n - 1] + [n // 2] * 5):
        t[(i * 97) % m] = v
    return t


# ---- f32 -> f16 ---------------------------------------------------------------------------------------------------------------------
def _f32_bits_of_pow2_multiple(v, e):
    """bits of the f32 value v * 2^e for an integer 1 <= v < 2^24 (exact: integer arithmetic only)."""
    p = v.bit_length() - 1
    return ((p + e + 127) << 23) | ((v - (1 << p)) << (23 - p))


def f16_patterns():
    """1023 positive finite f16 patterns h with a finite successor: subnormals, the subnormal / normal border, the top binade, and a
    spread over the ordinary exponents."""
    rng = np.random.default_rng(71)
    fixed = set(range(0, 128)) | set(range(0x3F0, 0x410)) | set(range(0x7BFE - 127, 0x7BFF))
    rest = [int(h) for h in rng.permutation(np.arange(0x410, 0x7B00)) if int(h) not in fixed]
    return sorted(fixed) + sorted(rest[:1023 - len(fixed)])


def f16_rounding_list():
    """(f32 bit patterns, expected f16 bit patterns), both by integer arithmetic.  For every pattern h of f16_patterns(): the exact
    midpoint of h and its successor (ties to the even pattern), the midpoint minus one f32 ulp (-> h) and plus one (-> h + 1), in both
    signs.  Then 2^-25 (ties to zero), its f32 successor (-> the smallest subnormal) and 65519.996, the largest f32 below the midpoint
    of 65504 and 2^16 (-> 65504).  Nothing rounds to infinity, nothing is NaN.  Padded with 1.0 to 2 x 48 x 64 values."""
    f32, f16 = [], []
    for h in f16_patterns():
        e, m = h >> 10, h & 0x3FF
        # midpoint of h and h + 1: (2 m + 1) * 2^-25 for a subnormal h, (2048 + 2 m + 1) * 2^(e - 26) otherwise
        mid = _f32_bits_of_pow2_multiple(2 * m + 1, -25) if e == 0 else _f32_bits_of_pow2_multiple(2048 + 2 * m + 1, e - 26)
        for bits, want in ((mid, h + (h & 1)), (mid - 1, h), (mid + 1, h + 1)):
            f32 += [bits, bits | 0x80000000]
            f16 += [want, want | 0x8000]
    top = _f32_bits_of_pow2_multiple(2048 + 2047, 30 - 26)          # 65520 = midpoint of 0x7BFF and 2^16
    f32 += [_f32_bits_of_pow2_multiple(1, -25), _f32_bits_of_pow2_multiple(1, -25) + 1, top - 1]
    f16 += [0, 1, 0x7BFF]
    while len(f32) < 2 * 48 * 64:
        f32.append(0x3F800000)
        f16.append(0x3C00)
    return np.array(f32, np.uint32), np.array(f16, np.uint16)


# ---- score model --------------------------------------------------------------------------------------------------------------------
# (d_emb, d_hidden, out_ch, batch); batch * d_hidden or batch * out_ch is no multiple of 4 in several: the last workgroup has idle waves
SCORE_SHAPES = [(1, 1, 1, 1), (63, 65, 1, 3), (65, 63, 3, 5), (100, 130, 2, 7), (1152, 128, 3, 1)]


def score_case(shape, saturated, seed=73):
    """up, bias, down, x.  Unsaturated: pre-activations of order 1 and down_proj scaled so that the outputs are of order 1.
    Saturated: |up . x| stays below 8 and the bias is +40 or -150 by turns, so every hidden pre-activation is >= 20 or <= -110:
    1 + expf(-s) is 1 or infinity in f32 whatever expf's last bits are, silu is the identity or -0, and the result depends only on the
    two dot64 sums that the kernel and the oracle state identically."""
    d_emb, d_hidden, out_ch, batch = shape
    rng = np.random.default_rng(seed + d_emb * 7 + d_hidden)
    up = (rng.standard_normal((d_hidden, d_emb)) / np.sqrt(d_emb)).astype(np.float32)
    x = rng.standard_normal((batch, d_emb)).astype(np.float32)
    if saturated:
        bias = np.where(np.arange(d_hidden) % 2 == 0, 40.0, -150.0).astype(np.float32)
        down = (rng.standard_normal((out_ch, d_hidden)) / np.sqrt(d_hidden)).astype(np.float32)
    else:
        bias = rng.standard_normal(d_hidden).astype(np.float32)
        down = (rng.standard_normal((out_ch, d_hidden)) * np.sqrt(d_hidden) / d_emb).astype(np.float32)
    return up, bias, down, x


def pre_activations_f64(up, bias, x):
    return x.astype(np.float64) @ up.astype(np.float64).T + bias.astype(np.float64)[None, :]


def score_batch_f64(up, bias, down, x):
    """score_model.rs:13-32 in float64 on the f32 inputs: down . silu(up . x + bias) * d_emb / d_hidden."""
    s = pre_activations_f64(up, bias, x)
    h = s / (1.0 + np.exp(-s))
    return h @ down.astype(np.float64).T * (up.shape[1] / up.shape[0])


# ---- descriptor buckets -------------------------------------------------------------------------------------------------------------
BUCKET_CDF_LENS = [1, 2, 3, 254, 255]
# (n_desc, rows): rows * n_desc = 1, 255, 257 where n_desc divides them (1 and 5); 4 divides none of the three, so the two row counts
# on either side of one 256-thread workgroup (252 and 260 scores), and 260 for n_desc = 5 as well
BUCKET_SHAPES = [(1, 1), (1, 255), (1, 257), (5, 51), (5, 52), (4, 63), (4, 65)]


def bucket_cdfs(n_desc, cdf_len, seed=79):
    """Ascending CDFs that contain 0.0 and runs of equal entries at the front, in the middle and at the end (as far as the length
    allows: [a, a] at two, [a, a, b] at three)."""
    rng = np.random.default_rng(seed + 10 * n_desc + cdf_len)
    cdfs = np.sort(rng.standard_normal((n_desc, cdf_len)).astype(np.float32), axis=1)
    for c in cdfs:
        if cdf_len >= 254:
            c[cdf_len // 3] = 0.0
            c[:] = np.sort(c)
            c[:3] = c[2]
            c[100:104] = c[103]
            c[-3:] = c[-3]
        elif cdf_len == 3:
            c[:] = (0.0, 0.0, abs(c[2]) + 0.5)
        else:
            c[:] = 0.0
    return cdfs


def bucket_scores(cdfs, n, seed=83):
    """[n, n_desc] scores drawn in turn from: entries of the channel's CDF, midpoints between neighbours, values below the first and
    above the last entry, +inf, -inf, NaN and -0.0."""
    n_desc, cdf_len = cdfs.shape
    rng = np.random.default_rng(seed + n + cdf_len)
    out = np.empty((n, n_desc), np.float32)
    for j, c in enumerate(cdfs):
        mids = ((c[:-1].astype(np.float64) + c[1:]) / 2).astype(np.float32) if cdf_len > 1 else np.array([c[0] + 1], np.float32)
        special = np.array([c[0] - 1, c[-1] + 1, np.inf, -np.inf, np.nan, -0.0, c[0], c[-1], c[cdf_len // 2]], np.float32)
        pool = np.concatenate([special, rng.permutation(c), rng.permutation(mids)])
        out[:, j] = pool[(np.arange(n) + 3 * j) % len(pool)]
    return out


def in_equal_run(cdfs, scores):
    """mask [n, n_desc]: the score equals an entry that occurs more than once in its channel's CDF."""
    out = np.zeros(scores.shape, bool)
    for j, c in enumerate(cdfs):
        vals, counts = np.unique(c, return_counts=True)
        out[:, j] = np.isin(scores[:, j], vals[counts > 1])
    return out
