"""tests/describe_ref.py (the numpy restatement of csrc/describe.hip) against numpy and the oracle, on the CPU: the interpolation is
numpy.quantile's bit for bit, the three-pass radix select is numpy.sort's order statistics on adversarial key sets, the bucket step is the
oracle's, and fma32 is fmaf.  tests/test_gpu_describe.py then holds the device to the restatement."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import describe_ref as ref
import pq_codec_cases as cases

SIZES = [1, 2, 3, 254, 255, 256, 70001]


def f32_normals(n, seed=1):
    return np.random.default_rng(seed + n).standard_normal(n).astype(np.float32)


def f32_ties(n, seed=2):
    """five distinct values: nearly every rank pair straddles equal keys, and the few boundaries fall between requested ranks.  (No
    -0.0: numpy's partition leaves -0.0 and +0.0 in either order and the select folds them, so only their value is comparable; the key
    sets below have both.)"""
    return np.random.default_rng(seed + n).choice(np.array([-1.5, -0.125, 0.0, 0.25, 3.0], np.float32), n)


def timestamps(n, seed=3):
    """seconds on both sides of 2^31 (2038), as int64"""
    return np.random.default_rng(seed + n).integers(2**31 - 10**6, 2**31 + 10**6, n).astype(np.int64)


def key_sets(n, seed=5):
    """name -> keys (f32, or u32 for the timestamp channel): the sets the select is checked on, here and on the device"""
    rng = np.random.default_rng(seed + n)
    base = np.float32(1.5).view(np.uint32)
    sets = {
        "equal": np.full(n, np.float32(-2.75)),
        "two values": np.where(np.arange(n) < (n + 1) // 2, np.float32(1.0), np.float32(-1.0)).astype(np.float32),
        "last 10 bits": (base + rng.integers(0, 1024, n).astype(np.uint32)).view(np.float32),
        "top 11 bits": (rng.integers(0, 2048, n).astype(np.uint32) << np.uint32(21)).view(np.float32),
        "around zero": rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, np.inf, -np.inf, 1.0, -1.0],
                                           np.float32), n),
        "normals": f32_normals(n),
        "timestamps": (rng.integers(-2**20, 2**20, n) + 2**31).astype(np.uint32),
    }
    top = sets["top 11 bits"]
    top[np.isnan(top)] = np.float32(0.5)            # exponent 255 with a mantissa bit: not a key
    rng.shuffle(sets["two values"])
    return sets


def ranks_for(n):
    """all n ranks up to 512 keys, else the 255-quantile pairs (duplicates included)"""
    if n <= 512:
        return np.arange(n, dtype=np.uint64)
    lo, hi, _ = ref.quantile_ranks(n)
    return np.concatenate([lo, hi]).astype(np.uint64)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("make", [f32_normals, f32_ties, timestamps])
def test_interpolation_is_numpy_quantile_bit_for_bit(make, n):
    x = make(n)
    want = np.quantile(x, np.linspace(0, 1, 255))
    got = ref.quantiles(x)
    assert want.dtype == np.float64 and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for cdf_len in (1, 3):
        assert np.array_equal(ref.quantiles(x, cdf_len).view(np.uint64), np.quantile(x, np.linspace(0, 1, cdf_len)).view(np.uint64))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 70001])
def test_radix_select_is_the_sorted_order(n):
    for name, x in key_sets(n).items():
        r = ranks_for(n)
        got, want = ref.radix_select(x, r), np.sort(x)[r.astype(np.int64)]
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    # the two-value boundary straddles a requested rank: both values come back
    two = ref.radix_select(key_sets(n)["two values"], ranks_for(n))
    assert n == 1 or (two.min(), two.max()) == (-1.0, 1.0)


def test_radix_select_refuses_nan_with_the_count():
    x = f32_normals(70001)
    x[[5, 60000]] = np.nan
    with pytest.raises(ValueError, match="2 NaN"):
        ref.radix_select(x, [0])


@pytest.mark.parametrize("cdf_len", cases.BUCKET_CDF_LENS)
def test_bucket_step_is_the_oracles(orc, cdf_len):
    cdfs = cases.bucket_cdfs(4, cdf_len)
    scores = cases.bucket_scores(cdfs, 65)
    assert np.array_equal(ref.descriptor_bytes(cdfs, scores), orc.descriptor_buckets(cdfs, scores))
    ts = timestamps(65)
    want = orc.descriptor_buckets(cdfs, np.concatenate([scores[:, :3], ts.astype(np.float32)[:, None]], axis=1))
    assert np.array_equal(ref.descriptor_bytes(cdfs, scores[:, :3], ts), want)


def test_fma32_is_fmaf():
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype, libm.fmaf.argtypes = C.c_float, [C.c_float] * 3
    rng = np.random.default_rng(7)
    n = 20000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (-a * b * (1 + rng.integers(-3, 4, n) * 2.0**-24)).astype(np.float32)      # heavy cancellation: the f64 sum is inexact
    c[::3] = rng.standard_normal(len(c[::3])).astype(np.float32)
    a[:4], b[:4], c[:4] = (0.0, -0.0, 1e-30, -1e-30), (1.0, 1.0, 1e-30, 1e-30), (0.0, -0.0, 0.0, 1e-45)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(ref.fma32(a, b, c).view(np.uint32), want.view(np.uint32))


def test_restated_scores_are_the_float64_scores_to_rounding():
    """the restated orders compute the score model: against float64 within the project's 1e-5 on an unsaturated case, and a saturated
    case's silu is the identity or -0 (so the device comparison there is about the sums alone)"""
    up, bias, down, x = cases.score_case((100, 130, 2, 7), saturated=False)
    x = x.astype(np.float16).astype(np.float32)
    got = ref.score_rows(up, bias, down, x).astype(np.float64)
    want = cases.score_batch_f64(up, bias, down, x)
    assert np.max(np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want))) <= 1.0
    up, bias, down, x = cases.score_case((65, 63, 3, 5), saturated=True)
    x = x.astype(np.float16).astype(np.float32)
    s = (ref.pre_activations(up, x) + bias[None, :]).astype(np.float32)
    h = ref.silu32(s)
    pos = s > 0
    assert np.array_equal(h[pos], s[pos]) and not h[~pos].any() and np.signbit(h[~pos]).all()
