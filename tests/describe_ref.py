"""numpy restatement of csrc/describe.hip: the fused score MLP in the kernel's own summation orders, the three-pass radix select, the
CDF fit (meme-rater/compute_cdf.py:64-71) and the bucket step (src/dump_processor.rs:483-491).  tests/test_describe_host.py holds
these to numpy and the oracle on the CPU; tests/test_gpu_describe.py holds the device to them.

The orders, as the header of csrc/describe.hip states them:
  pre-activation   s[b][n] = fma(up[n][K-1], x[b][K-1], ... fma(up[n][0], x[b][0], 0)): one f32 fma chain, k ascending (the f32 MFMA)
  bias             s += bias[n]                              one f32 add
  silu             h = s / (1 + expf(-s))
  hidden sum       the hidden units are walked in tiles of HID_TILE = 128, a tile in two halves of 64 (w = 0, 1).  Per output channel c,
                   for the half (tile t, w) with units n_j = 128 t + 64 w + j:
                       u_j = fma(h[n_{j+32}], down[c][n_{j+32}], h[n_j] * down[c][n_j])      j < 32   (units past d_hidden give +0)
                       S   = the xor butterfly over u_0 .. u_31: five rounds v_j = v_j + v_{j ^ o}, o = 1, 2, 4, 8, 16
                       T_w = T_w + S                                                      t ascending, from +0
  scale            score = (T_0 + T_1) * (f32(d_emb) / f32(d_hidden))   (src/score_model.rs:16)
Nothing in them names the row's place in the call, the number of rows or the grid."""
import numpy as np

ROW_TILE = 128     # rows per workgroup
HID_TILE = 128     # hidden units per step of a workgroup, summed in two halves of 64
K_STEP = 32        # k per LDS stage


def fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays, exactly: the product of two f32 is exact in f64; the f64 sum is rounded to odd (TwoSum gives the
    rounding error, an inexact even result moves one f64 ulp towards it), after which the narrowing to f32 rounds once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)                      # the exact sum lies further from zero than s
    bits[fix & away] += 1
    bits[fix & ~away] -= 1
    with np.errstate(over="ignore"):
        return bits.view(np.float64).astype(np.float32)


def pre_activations(up, x):
    """[rows, d_hidden] f32: the k-ascending fma chain from 0."""
    up, x = np.asarray(up, np.float32), np.asarray(x, np.float32)
    s = np.zeros((x.shape[0], up.shape[0]), np.float32)
    for k in range(up.shape[1]):
        s = fma32(x[:, k:k + 1], up[None, :, k], s)
    return s


def silu32(s, expf=None):
    """s / (1 + expf(-s)) in f32; expf defaults to numpy's (any expf gives the same bits where 1 + expf(-s) is 1 or infinity)."""
    s = np.asarray(s, np.float32)
    with np.errstate(over="ignore"):
        e = (np.exp(-s) if expf is None else expf(-s)).astype(np.float32)
        return (s / (np.float32(1.0) + e)).astype(np.float32)


def hidden_sum(h, down, d_emb):
    """[rows, out_channels] f32 from the activations h [rows, d_hidden], in the stated order."""
    h, down = np.asarray(h, np.float32), np.asarray(down, np.float32)
    rows, d_hidden = h.shape
    n_tiles = -(-d_hidden // HID_TILE)
    hp = np.zeros((rows, n_tiles * HID_TILE), np.float32)
    hp[:, :d_hidden] = h
    hp = hp.reshape(rows, n_tiles, 2, 2, 32)                 # [row, tile, half w, j / 32, j % 32]
    lanes = np.arange(32)
    out = np.empty((rows, down.shape[0]), np.float32)
    scale = np.float32(d_emb) / np.float32(d_hidden)
    for c in range(down.shape[0]):
        dp = np.zeros(n_tiles * HID_TILE, np.float32)
        dp[:d_hidden] = down[c]
        dp = dp.reshape(1, n_tiles, 2, 2, 32)
        v = fma32(hp[:, :, :, 1], dp[:, :, :, 1], (hp[:, :, :, 0] * dp[:, :, :, 0]).astype(np.float32))
        for o in (1, 2, 4, 8, 16):
            v = (v + v[..., lanes ^ o]).astype(np.float32)
        S = v[..., 0]                                        # [row, tile, w]; every lane holds the same sum
        T = np.zeros((rows, 2), np.float32)
        for t in range(n_tiles):
            T = (T + S[:, t]).astype(np.float32)
        out[:, c] = (T[:, 0] + T[:, 1]).astype(np.float32) * scale
    return out


def score_rows(up, bias, down, x):
    """The device's scores of the f32 rows x (the exact widenings of the f16 rows), bit for bit where silu is saturated."""
    s = (pre_activations(up, x) + np.asarray(bias, np.float32)[None, :]).astype(np.float32)
    return hidden_sum(silu32(s), down, np.asarray(up).shape[1])


# ---- radix select ---------------------------------------------------------------------------------------------------------------------
DIGIT_BITS = (11, 11, 10)


def keys_of(x):
    """u32 keys whose unsigned order is the ascending order of x: u32 as it is; f32 through the order-preserving transform with -0.0
    folded onto +0.0.  NaNs are refused, counted."""
    x = np.asarray(x)
    if x.dtype == np.uint32:
        return x.copy()
    assert x.dtype == np.float32
    n_nan = int(np.isnan(x).sum())
    if n_nan:
        raise ValueError("%d NaN among the keys" % n_nan)
    b = x.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b >> 31).astype(bool)
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def values_of(keys, dtype):
    keys = np.asarray(keys, np.uint32)
    if dtype == np.uint32:
        return keys
    b = np.where((keys >> 31).astype(bool), keys & np.uint32(0x7FFFFFFF), ~keys).astype(np.uint32)
    return b.view(np.float32)


def radix_select(x, ranks):
    """np.sort(x)[ranks] by three digit histograms (11 / 11 / 10 bits), never sorting: per pass, count the digit among the keys whose
    prefix is a selected one, and descend each rank into the bucket that holds it."""
    x = np.asarray(x)
    keys = keys_of(x)
    ranks = np.asarray(ranks, np.uint64)
    assert ranks.size == 0 or int(ranks.max()) < keys.size
    prefix = np.zeros(ranks.size, np.uint32)
    rem = ranks.astype(np.int64)
    shift = 32
    for bits in DIGIT_BITS:
        shift -= bits
        digit = (keys >> np.uint32(shift)) & np.uint32((1 << bits) - 1)
        upper = (keys.astype(np.uint64) >> np.uint64(shift + bits)).astype(np.uint32)
        for p in np.unique(prefix):
            hist = np.bincount(digit[upper == p], minlength=1 << bits)
            ends = np.cumsum(hist)
            for i in np.nonzero(prefix == p)[0]:
                d = int(np.searchsorted(ends, rem[i], side="right"))
                rem[i] -= ends[d] - hist[d]
                prefix[i] = (p << bits) | d
    return values_of(prefix, x.dtype)


# ---- CDF fit --------------------------------------------------------------------------------------------------------------------------
def quantile_ranks(n, cdf_len=255):
    """(lo, hi, gamma): numpy's linear method -- q = linspace(0, 1, cdf_len), v = (n - 1) q, lo = floor(v), hi = min(lo + 1, n - 1)."""
    v = (n - 1) * np.linspace(0, 1, cdf_len)
    lo = np.floor(v)
    gamma = v - lo
    lo = lo.astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1), gamma


def interpolate(a, b, gamma):
    """numpy's _lerp on the two order statistics: b - a is taken in the type of the data (one f32 subtraction for a score channel, exact
    for integer timestamps), everything after it in float64."""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (b - a).astype(np.float64)
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.where(gamma >= 0.5, b - d * (1 - gamma), a + d * gamma)


def quantiles(x, cdf_len=255):
    """numpy.quantile(x, linspace(0, 1, cdf_len)) in float64 from the order statistics alone (a sort stands in for the select)."""
    x = np.sort(np.asarray(x))
    lo, hi, gamma = quantile_ranks(x.size, cdf_len)
    return interpolate(x[lo], x[hi], gamma)


def fit_cdfs(scores, timestamps=None, cdf_len=255):
    """f32 [channels (+1), cdf_len]: the descriptor_cdfs of index.msgpack for these scores."""
    scores = np.asarray(scores, np.float32)
    chans = [quantiles(scores[:, c], cdf_len) for c in range(scores.shape[1])]
    if timestamps is not None:
        chans.append(quantiles(np.asarray(timestamps, np.int64), cdf_len))
    return np.stack(chans).astype(np.float32)


# ---- bucket step ----------------------------------------------------------------------------------------------------------------------
def bucket(cdf, s):
    """core::slice::binary_search_by(|x| x.partial_cmp(&s)) as Rust 1.7x runs it: Ok(p) or Err(p) -> p."""
    size, base = len(cdf), 0
    if size == 0:
        return 0
    while size > 1:
        half = size // 2
        mid = base + half
        base = base if cdf[mid] > s else mid
        size -= half
    c = cdf[base]
    return base if c == s else base + (1 if c < s else 0)


def descriptor_bytes(cdfs, scores, timestamps=None):
    """u8 [n, channels (+1)]: bucket(cdfs[j], value_j), the timestamp as f32 (dump_processor.rs:481, `as f32`)."""
    cdfs, scores = np.asarray(cdfs, np.float32), np.asarray(scores, np.float32)
    vals = scores if timestamps is None else np.concatenate([scores, np.asarray(timestamps).astype(np.float32)[:, None]], axis=1)
    out = np.empty(vals.shape, np.uint8)
    for i in range(vals.shape[0]):
        for j in range(vals.shape[1]):
            out[i, j] = bucket(cdfs[j], vals[i, j])
    return out
