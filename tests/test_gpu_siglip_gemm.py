"""The SigLIP GEMM family against float64, element by element: every kernel launch_gemm / launch_gemm_fused can pick (gemm_kernel,
gemm8p_kernel, the four forms of gemm8pp_kernel, gemm_skinny_kernel, gemm_mid_kernel with and without the K split) and every epilogue
(BF16, GELU in both flavours, RESID, PATCH, the QKV scatter, PART, and the LayerNorm-fused consumers and producer with
fold_ln_weights_kernel, row_stats_kernel and ln_stats_finalize_kernel around them).

Everything goes through mse_debug_siglip_gemm / mse_debug_siglip_gemm_fused: ONE launch as the towers make it, so the kernel is the
one production picks; dispatch() below restates the thresholds (a CPU test pins them to the source, another shows which case reaches
which kernel).  The reference is float64 numpy over the operands as the hook rounds them (bf16_round / f16_round restate that).

Bounds, per element, from the operands and the reference only.  S = sum_k |x_k w_nk|, pre = the exact pre-activation:
    E          = 2 K 2^-24 S + 2^-23 |pre|                 fp32 accumulation in any order (x 2: the matrix cores' rounding), bias add
    BF16, QKV  E + U16 (|ref| + E)                          U16 = 2^-8: bf16 keeps 8 significant bits, so round-to-nearest is off by
                                                            up to 2^-8 |v| (test_unit_roundoffs: 2^-9 fails on the rounding alone)
    GELU       B = 1.13 E + 2.6e-5 + 2^-20 |pre|;  B + U16 (|ref| + B)       (1.13 >= |gelu'|; 2.6e-5: the fit; 2^-20: exp2, rcp)
    PATCH      E + 2^-24 |ref| (the position add) + 2^-11 (|ref| + E)        fp16 store
    RESID      E + 2^-23 |ref|                                               the fp32 add and store
    PART       per slab 2 (K / ksplit) 2^-24 S_slab + 2^-23 |ref_slab|
    RESID_LN   d = E + U16 (|pre| + E)   (the branch is staged as bf16);  d + 2^-24 |ref| + 2^-11 (|ref| + d)
    consumers  see consumer_reference()
The integer family (entries in [-8, 8], integer bias: every partial sum exact in fp32, so its E is 0) has NO tolerance: the output
must be the correctly rounded exact value, bit for bit (GELU and the fused consumers, which are not exact, keep their bound with
E = 0).  The producer stages its branch as bf16 before the add, so its integer operands are sparse enough for |pre| <= 256.

Not reachable: N = 32 for the skinny kernel -- launch_gemm refuses N % 128 != 0, and so does the hook (asserted); N = 128 is four of
its 32-column workgroups.

The largest |got - ref| / bound measured per kernel and family is kept in DESIGN 3.4.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

BF16, GELU, RESID, PATCH, QKV, RESID_LN, PART = range(7)
EPI_NAME = ["BF16", "GELU", "RESID", "PATCH", "QKV", "RESID_LN", "PART"]
U16 = 2.0 ** -8        # unit roundoff of bf16 (8 significant bits)
UH = 2.0 ** -11        # of fp16 (11)
GELU_FIT = 2.6e-5      # stated at gelu_coef
DH = 72
HEADS = 16             # the towers: 16 heads of 72
D = HEADS * DH
CSRC = os.path.join(ROOT, "meme-search-engine_amd", "csrc")


def round_up(v, m):
    return (v + m - 1) // m * m


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def f16_round(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


SENT_BF16 = np.array([0xA5A5 << 16], np.uint32).view(np.float32)[0]
SENT_F16 = np.array([0xA5A5], np.uint16).view(np.float16).astype(np.float32)[0]
SENT_F32 = np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0]


# ---------------------------------------------------------------------------------------------------------
# kernel selection, restated from launch_gemm / launch_gemm_t (siglip_kernels.hip); test_thresholds_match_the_source pins the numbers
# ---------------------------------------------------------------------------------------------------------
SMALL_SKINNY_ROWS, SMALL_MID_ROWS, SMALL_T128_ROWS = 64, 3072, 2048
SPLIT_MAX_ROWS, SPLIT_T128_ROWS, SK_NW = 768, 384, 12
PP_MIN_K, PERSIST_MIN_K = 128, 256


def dispatch(epi, rows, N, K, skinny):
    """[(kernel, first column, end column, what happens to rows rows .. M)] of one launch_gemm call.  Padding: ("zero", t) rows up
    to the next multiple of t are zeroed and the rest kept; "keep"; "finite" (overwritten by an unconditional store)."""
    M = round_up(rows, 256)
    store_only = epi in (BF16, GELU)
    if epi == PART:
        t = 128 if rows > SPLIT_T128_ROWS else 64
        return [("mid%d<PART>" % t, 0, N, ("raw", t))]
    if skinny:
        pick = skinny if skinny >= 2 else (2 if rows <= SMALL_SKINNY_ROWS else
                                           ((4 if rows > SMALL_T128_ROWS and K > 2048 else 3) if rows <= SMALL_MID_ROWS else 0))
        if pick == 2:
            return [("skinny<R%d>" % (3 if K // 32 <= 3 * SK_NW else 4), 0, N, ("zero", 64) if store_only else "keep")]
        if pick in (3, 4):
            t = 64 if pick == 3 else 128
            return [("mid%d" % t, 0, N, ("zero", t) if store_only else "keep")]
    zero_m = ("zero", M) if store_only else "keep"
    n256 = N // 256 * 256 if K >= PP_MIN_K else 0
    persist = K >= PERSIST_MIN_K
    out = []
    if n256:
        if epi in (BF16, GELU):
            out.append(("pp256" if persist else "8p", 0, n256, "finite" if persist else zero_m))
        elif epi == QKV:
            nqk = min(2 * D, n256)
            out.append(("pp256<QKV>" if persist else "8p<QKV>", 0, nqk, "finite" if persist else "keep"))
            if n256 > nqk:
                out.append(("pp256<QKV,vswap>" if persist else "8p<QKV,vswap>", nqk, n256, "finite" if persist else "keep"))
        else:
            out.append(("8p", 0, n256, "keep"))
    if n256 < N:
        if epi in (BF16, QKV) and N - n256 == 128 and persist and (epi == BF16 or n256 >= 2 * D):
            out.append(("pp128<QKV,vswap>" if epi == QKV else "pp128", n256, N, "finite"))
        else:
            out.append(("gen1", n256, N, zero_m))
    return out


# ---------------------------------------------------------------------------------------------------------
# the cases (rows, N, K, epi, skinny, extra)
# ---------------------------------------------------------------------------------------------------------
def _c(rows, N, K, epi, skinny, **kw):
    return (rows, N, K, epi, skinny, tuple(sorted(kw.items())))


def case_id(c):
    rows, N, K, epi, skinny, extra = c
    return "%s-r%d-n%d-k%d-s%d%s" % (EPI_NAME[epi], rows, N, K, skinny, "".join("-%s%s" % kv for kv in extra))


SKINNY_CASES = (
    [_c(37, 128, K, BF16, 1) for K in (64, 1088, 1152, 1216, 4352)] +
    [_c(r, 128, K, BF16, 1) for r in (1, 64) for K in (1152, 1216)] +
    [_c(64, 1152, 1152, BF16, 1), _c(64, 1152, 4352, BF16, 1), _c(1, 1152, 1088, GELU, 1), _c(37, 128, 1152, GELU, 1),
     _c(37, 128, 1152, GELU, 1, tanh=1), _c(37, 128, 1216, RESID, 1), _c(64, 128, 1088, PATCH, 1, tokens=64)])
MID_CASES = (
    [_c(r, 256, 1152, BF16, 1) for r in (65, 100, 736)] +
    [_c(100, 256, K, BF16, 1) for K in (64, 128, 192, 256)] +
    [_c(100, 256, 1152, GELU, 1), _c(100, 256, 192, RESID, 1), _c(736, 128, 128, PATCH, 1, tokens=736),
     _c(2049, 128, 4352, BF16, 1), _c(2944, 128, 4352, BF16, 1), _c(2944, 128, 4352, GELU, 1), _c(2049, 128, 1152, BF16, 1),
     _c(333, 256, 320, BF16, 3), _c(333, 256, 320, BF16, 4), _c(333, 256, 320, GELU, 4), _c(333, 256, 320, RESID, 3)])
PART_CASES = [_c(100, 1152, 4352, PART, 1, ksplit=4), _c(736, 1152, 4352, PART, 1, ksplit=4), _c(384, 128, 4352, PART, 1, ksplit=4),
              _c(385, 128, 4352, PART, 1, ksplit=4), _c(64, 1152, 1152, PART, 1, ksplit=3)]
LARGE_CASES = (
    [_c(M, N, K, epi, 0) for (M, N) in ((256, 384), (256, 256), (512, 384)) for K in (64, 128, 192, 256, 320, 1152) for epi in (BF16, GELU)] +
    [_c(256, 384, 320, GELU, 0, tanh=1)] +
    [_c(256, 384, K, RESID, 0) for K in (128, 640)] + [_c(256, 384, K, PATCH, 0, tokens=96) for K in (128, 640)] +
    [_c(5, 384, 640, RESID, 0), _c(255, 384, 640, RESID, 0), _c(255, 384, 64, RESID, 0), _c(1472, 384, 128, PATCH, 0, tokens=736)])
QKV_CASES = (
    [_c(rows, 3 * D, K, QKV, 0, tokens=t) for (rows, t) in ((256, 64), (768, 64), (736, 736)) for K in (256, 1152)] +
    [_c(256, 3 * D, 128, QKV, 0, tokens=64), _c(256, 3 * D, 64, QKV, 0, tokens=64), _c(728, 3 * D, 256, QKV, 0, tokens=729),
     _c(64, 3 * D, 1152, QKV, 1, tokens=64), _c(736, 3 * D, 1152, QKV, 1, tokens=736)])
SEAM_CASES = [_c(8192, 4352, 256, BF16, 0), _c(8192, 4352, 256, GELU, 0)]
PLAIN_CASES = SKINNY_CASES + MID_CASES + PART_CASES + LARGE_CASES + QKV_CASES

# kernels the issue asks every suite run to reach
REQUIRED_KERNELS = {"skinny<R3>", "skinny<R4>", "mid64", "mid128", "mid64<PART>", "mid128<PART>", "gen1", "8p", "pp256", "pp128",
                    "8p<QKV>", "8p<QKV,vswap>", "pp256<QKV>", "pp256<QKV,vswap>", "pp128<QKV,vswap>"}


# ---------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def operands(family, rows, N, K, epi, extra):
    """x [rows][K], w [N][K] (bf16 values as float32), bias [N], and per epilogue resid / pos -- exactly what the kernel multiplies."""
    kw = dict(extra)
    rng = np.random.default_rng([rows, N, K, epi, sum(map(ord, family))])
    aux = {}
    if family == "int":
        x = rng.integers(-8, 9, (rows, K)).astype(np.float32)
        w = rng.integers(-8, 9, (N, K)).astype(np.float32)
        bias = rng.integers(-16, 17, N).astype(np.float32)
        if epi == RESID:
            aux["resid"] = rng.integers(-64, 65, (rows, N)).astype(np.float32)
        if epi == PATCH:
            aux["pos"] = rng.integers(-16, 17, (kw["tokens"], N)).astype(np.float32)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
        w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
        bias = (rng.standard_normal(N) * math.sqrt(0.1)).astype(np.float32)
        if family == "heavy" and epi != GELU:
            # two pairs of columns with equal x of magnitude 50-200 and opposite large w: sum |x w| is hundreds of times |sum x w|
            cols = rng.choice(K, 4, replace=False)
            for a, b in (cols[:2], cols[2:]):
                x[:, a] = x[:, b] = rng.uniform(50, 200, rows) * rng.choice([-1, 1], rows)
                w[:, a] = rng.standard_normal(N) * 1.0
                w[:, b] = -bf16_round(w[:, a]) + (rng.standard_normal(N) * 2.0 ** -9).astype(np.float32)
        if family == "heavy" and epi == GELU:
            # pre-activations across [-12, 12] (the x^2 clamp at 50 is |x| = 7.07), every fourth column within |x| < 0.01
            w *= np.float32(0.004)
            bias = np.linspace(-12, 12, N).astype(np.float32)
            bias[::4] = 0.0
        if epi == RESID:
            aux["resid"] = rng.standard_normal((rows, N)).astype(np.float32)
        if epi == PATCH:
            aux["pos"] = (rng.standard_normal((kw["tokens"], N)) * 0.5).astype(np.float32)
    x, w = bf16_round(x), bf16_round(w)
    for a in (x, w, bias, *aux.values()):
        a.setflags(write=False)
    return x, w, bias, aux


def gelu_exact(x, tanh):
    x = np.asarray(x, np.float64)
    if tanh:
        return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    import torch
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())


def gelu_kernel_formula(x, tanh):
    """gelu2 (siglip_kernels.hip) in float64: x / (1 + exp(-x (a + b s + c s^2))), s = min(x^2, 50)."""
    a, b, c = (1.5957691216, 0.0713548163, 0.0) if tanh else (1.59501574, 7.40113143e-02, -7.03036941e-04)
    x = np.asarray(x, np.float64)
    s = np.minimum(x * x, 50.0)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x * ((c * s + b) * s + a)))


def accumulation_bound(family, K, ax, aw, pre):
    """E.  The integer family's partial sums and bias add are exact in fp32 (|pre| < 2^24): its E is 0."""
    if family == "int":
        assert np.abs(pre).max() < 2 ** 24
        return np.zeros_like(pre)
    return 2 * K * 2.0 ** -24 * (ax @ aw.T) + 2.0 ** -23 * np.abs(pre)


@functools.lru_cache(maxsize=2)
def reference(family, rows, N, K, epi, extra):
    """(ref, bound, exact): the float64 value of every output element of the real rows, its bound, and -- integer family, every
    epilogue but GELU -- the correctly rounded value the output must equal bit for bit.  PART: per slab, shape [ksplit][rows][N]."""
    kw = dict(extra)
    x, w, bias, aux = operands(family, rows, N, K, epi, extra)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ax, aw = np.abs(x64), np.abs(w64)
    if epi == PART:
        ks = kw["ksplit"]
        step = K // ks
        ref = np.stack([x64[:, s * step:(s + 1) * step] @ w64[:, s * step:(s + 1) * step].T for s in range(ks)])
        S = np.stack([ax[:, s * step:(s + 1) * step] @ aw[:, s * step:(s + 1) * step].T for s in range(ks)])
        bound = (0.0 if family == "int" else 2 * step * 2.0 ** -24 * S) + 2.0 ** -23 * np.abs(ref)
        return ref, bound, (ref.astype(np.float32) if family == "int" else None)
    pre = x64 @ w64.T + bias.astype(np.float64)
    E = accumulation_bound(family, K, ax, aw, pre)
    exact = None
    if epi in (BF16, QKV):
        ref, bound = pre, E + U16 * (np.abs(pre) + E)
        exact = bf16_round(pre.astype(np.float32)) if family == "int" else None
    elif epi == GELU:
        ref = gelu_exact(pre, kw.get("tanh", 0))
        B = 1.13 * E + GELU_FIT + 2.0 ** -20 * np.abs(pre)
        bound = B + U16 * (np.abs(ref) + B)
    elif epi == PATCH:
        tok = np.arange(rows) % kw["tokens"]
        ref = pre + aux["pos"].astype(np.float64)[tok]
        bound = E + 2.0 ** -24 * np.abs(ref) + UH * (np.abs(ref) + E)
        exact = f16_round(ref.astype(np.float32)) if family == "int" else None
    else:
        ref = pre + aux["resid"].astype(np.float64)
        bound = E + 2.0 ** -23 * np.abs(ref)
        exact = ref.astype(np.float32) if family == "int" else None
    return ref, bound, exact


# ---------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def gemm_args(rows, N, K, epi, skinny, extra, flags=0, n_valid=0):
    from mse import ffi
    kw = dict(extra)
    a = ffi.DebugSiglipGemmArgs()
    a.rows, a.N, a.K, a.epi, a.skinny, a.gelu_tanh, a.flags, a.n_valid = rows, N, K, epi, skinny, kw.get("tanh", 0), flags, n_valid
    a.tokens, a.ksplit = kw.get("tokens", 0), kw.get("ksplit", 0)
    if epi == QKV:
        a.heads, a.dh = HEADS, DH
    return a


def run_gemm(case, x, w, bias, aux, flags=0, n_valid=0):
    """One hook call; returns the whole destinations (padding included) as float32 arrays."""
    from mse import ffi
    rows, N, K, epi, skinny, extra = case
    a = gemm_args(rows, N, K, epi, skinny, extra, flags, n_valid)
    L = ffi.lib()
    ffi.check(L.mse_debug_siglip_gemm(C.byref(a)), "mse_debug_siglip_gemm (sizes)")
    keep = [np.ascontiguousarray(v, np.float32) for v in (x, w, bias)]
    a.x, a.w, a.bias = (_p(v) for v in keep)
    for name in ("resid", "pos"):
        if name in aux:
            keep.append(np.ascontiguousarray(aux[name], np.float32))
            setattr(a, name, _p(keep[-1]))
    res = {}
    if epi == QKV:
        mats = a.n_seq * HEADS
        res["q"] = np.full((mats, a.n_pad, a.dh_pad), np.nan, np.float32)
        res["k"] = np.full((mats, a.n_pad, a.kdh_pad), np.nan, np.float32)
        res["vt"] = np.full((mats, a.dv_pad, a.n_pad), np.nan, np.float32)
        a.q, a.k, a.vt = _p(res["q"]), _p(res["k"]), _p(res["vt"])
    elif epi == PART:
        res["out"] = np.full((a.ksplit, a.slab_rows, N), np.nan, np.float32)
        a.out = _p(res["out"])
    else:
        res["out"] = np.full((a.M, N), np.nan, np.float32)
        a.out = _p(res["out"])
    ffi.check(L.mse_debug_siglip_gemm(C.byref(a)), "mse_debug_siglip_gemm " + case_id(case))
    res["args"] = a
    return res


def ratios(got, ref, bound):
    diff = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / bound)      # a zero bound (integer family, exact zero) admits only the exact value
    return np.where(np.isfinite(ratio), ratio, np.inf)


def worst(got, ref, bound):
    ratio = ratios(got, ref, bound)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), "worst at %s: got %.9g, reference %.9g, bound %.3g" % (list(map(int, i)), got[i], ref[i], bound[i])


def assert_same_bits(a, b, what):
    d = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert d.size == 0, "%s: %d elements differ, the first at %s: %r against %r" % (what, len(d), d[0].tolist(), a[tuple(d[0])], b[tuple(d[0])])


def scatter_qkv(a, values, fill):
    """What the QKV epilogue leaves of `values` [rows][3 D] in sentinel-filled (q, k, vt): row m is token m % n_pad of sequence m // n_pad."""
    rows = values.shape[0]
    mats = a.n_seq * HEADS
    q = np.full((mats, a.n_pad, a.dh_pad), fill, values.dtype)
    k = np.full((mats, a.n_pad, a.kdh_pad), fill, values.dtype)
    vt = np.full((mats, a.dv_pad, a.n_pad), fill, values.dtype)
    m = np.arange(rows)
    v = values.reshape(rows, 3, HEADS, DH)
    for h in range(HEADS):
        mat = (m // a.n_pad) * HEADS + h
        q[mat, m % a.n_pad, :DH] = v[:, 0, h]
        k[mat, m % a.n_pad, :DH] = v[:, 1, h]
        vt[mat[:, None], np.arange(DH)[None, :], (m % a.n_pad)[:, None]] = v[:, 2, h]
    return q, k, vt


def qkv_masks(a, rows):
    """(real, padding-row) masks over (q, k, vt): entries of rows < rows, entries of rows rows .. M."""
    ones = np.ones((a.M, 3 * D), np.float32)
    ones[rows:] = 2.0
    marks = scatter_qkv(a, ones, 0.0)
    return [mk == 1.0 for mk in marks], [mk == 2.0 for mk in marks]


def check_qkv(clean, dirty, rows, ref, bound, exact, overwritten, what):
    """q, K and Vt of a QKV launch, every element at its documented address: the real rows against the reference (bit for bit
    against `exact` where given); what is never written -- columns dh .. of q / K rows, Vt's row-sum row and the rows above it, every
    entry of no row below M -- still the sentinel; the entries of rows rows .. M overwritten with finite values in the columns whose
    kernel stores unconditionally (`overwritten` [3 D]), untouched in the others; with garbage in x's padding rows (`dirty`) the real
    entries keep their bits and everything stays finite."""
    a = clean["args"]
    real, pad = qkv_masks(a, rows)
    refs, bounds = scatter_qkv(a, ref, 0.0), scatter_qkv(a, bound, 1.0)
    exacts = scatter_qkv(a, exact, SENT_BF16) if exact is not None else None
    skipped = scatter_qkv(a, np.broadcast_to(~overwritten, (a.M, 3 * D)).astype(np.float32), 0.0)
    for j, name in enumerate(("q", "k", "vt")):
        got = clean[name]
        assert np.isfinite(got).all() and np.isfinite(dirty[name]).all(), "%s %s: a non-finite value" % (what, name)
        ratio, where = worst(np.where(real[j], got, 0.0), refs[j], bounds[j])
        print("%s %-2s largest |got - ref| / bound %.3f; %s" % (what, name, ratio, where))
        assert ratio <= 1.0, "%s %s: %s" % (what, name, where)
        if exacts is not None:
            assert_same_bits(np.where(real[j], got, SENT_BF16), exacts[j], "%s %s (integer family)" % (what, name))
        untouched = ~real[j] & ~pad[j]
        if name == "vt":
            assert (got[:, DH, :] == 1.0).all() and (got[:, DH + 1:, :] == SENT_BF16).all(), what
            untouched[:, DH, :] = False
        else:
            assert (got[:, :, DH:] == SENT_BF16).all(), what
        for res in (got, dirty[name]):
            assert (res[untouched] == SENT_BF16).all(), "%s %s: an entry of no row below M was written" % (what, name)
            assert (res[pad[j] & (skipped[j] == 1.0)] == SENT_BF16).all(), "%s %s: a kernel that skips rows >= m_valid wrote one" % (what, name)
        assert_same_bits(np.where(real[j], dirty[name], 0.0), np.where(real[j], got, 0.0), "%s %s: x padding reached real rows" % (what, name))


def check_padding(case, out, what, n_valid=None):
    """Rows rows .. M of a [M][N] destination against what the hook comment says the chosen kernels may do to them.  (Columns
    n_valid .. N of a run with garbage weight rows hold garbage products, which an fp16 store may carry to infinity.)"""
    rows, N, K, epi, skinny, extra = case
    sent = {BF16: SENT_BF16, GELU: SENT_BF16, PATCH: SENT_F16, RESID: SENT_F32}[epi]
    assert np.isfinite(out[:, :n_valid]).all(), what + ": a non-finite value"
    for kernel, c0, c1, mode in dispatch(epi, rows, N, K, skinny):
        pad = out[rows:, c0:c1]
        if mode == "keep":
            assert (pad == sent).all(), "%s: %s wrote to padding rows it must skip" % (what, kernel)
        elif mode == "finite":
            pass
        else:
            edge = round_up(rows, mode[1]) - rows
            assert (pad[:edge] == 0).all(), "%s: %s left rows below its tile edge unzeroed" % (what, kernel)
            assert (pad[edge:] == sent).all(), "%s: %s wrote above its tile edge" % (what, kernel)


# ---------------------------------------------------------------------------------------------------------
# CPU-only checks: thresholds, coverage, the GELU fit, the bounds are not vacuous, the hook refuses what the launchers refuse
# ---------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_thresholds_match_the_source():
    """dispatch() restates launch_gemm_t; a moved threshold must fail here instead of silently un-testing a kernel."""
    src = _source("siglip_kernels.hip")
    consts = dict(re.findall(r"(SMALL_SKINNY_ROWS|SMALL_MID_ROWS|SMALL_T128_ROWS|SPLIT_MAX_ROWS|SPLIT_T128_ROWS|SK_NW) = (\d+)", src))
    assert {k: int(v) for k, v in consts.items()} == dict(SMALL_SKINNY_ROWS=SMALL_SKINNY_ROWS, SMALL_MID_ROWS=SMALL_MID_ROWS,
                                                          SMALL_T128_ROWS=SMALL_T128_ROWS, SPLIT_MAX_ROWS=SPLIT_MAX_ROWS,
                                                          SPLIT_T128_ROWS=SPLIT_T128_ROWS, SK_NW=SK_NW)
    for line in (
            "if (a.K / 32 <= 3 * SK_NW) {",
            "else if (rows <= SMALL_SKINNY_ROWS) pick = 2;",
            "else if (rows <= SMALL_MID_ROWS) pick = (rows > SMALL_T128_ROWS && a_in.K > 2048) ? 4 : 3;",
            "const bool pp_ok = a_in.K >= %d &&" % PP_MIN_K,
            "const bool persist = !nopersist && a.K >= %d;" % PERSIST_MIN_K,
            "if (!narrow_off && a.N == 128 && a.K >= %d && qkv_ok) {" % PERSIST_MIN_K,
            "const int n256 = use256 ? (a_in.N / B2) * B2 : 0;",
            "const int tb = g.m_valid > SPLIT_T128_ROWS ? 128 : 64;",
            "constexpr bool store_only = EPI == EPI_BF16 || EPI == EPI_GELU || EPI == EPI_QKV;",
            "if constexpr (EPI == EPI_BF16 || EPI == EPI_QKV) {",
            "if (rows <= 0 || rows > SPLIT_MAX_ROWS || K < 2048 || (K / BK) % 4 || N % 128 || K % BK) return 1;",
            "constexpr int BM = 256, BN = 128, BK = 64, GW = 8, GS = 3;",
            "constexpr int B2 = 256, BK2 = 32;"):
        assert line in src, "launch_gemm changed: %r is gone -- update dispatch() and the cases with it" % line


def test_every_dispatch_branch_has_a_case(capsys):
    reached = {}
    for c in PLAIN_CASES + SEAM_CASES:
        rows, N, K, epi, skinny, extra = c
        for kernel, *_ in dispatch(epi, rows, N, K, skinny):
            reached.setdefault(kernel, []).append(case_id(c))
    with capsys.disabled():
        for kernel in sorted(reached):
            print("\n%-18s %3d cases, e.g. %s" % (kernel, len(reached[kernel]), ", ".join(reached[kernel][:3])), end="")
        print()
    assert REQUIRED_KERNELS <= set(reached), "no case reaches %s" % sorted(REQUIRED_KERNELS - set(reached))
    epis = {(k, c[3]) for c in PLAIN_CASES for k, *_ in dispatch(c[3], c[0], c[1], c[2], c[4])}
    for need in (("skinny<R3>", GELU), ("skinny<R4>", RESID), ("skinny<R3>", PATCH), ("skinny<R3>", QKV), ("mid64", QKV), ("mid64", GELU),
                 ("mid64", RESID), ("mid64", PATCH), ("mid128", GELU), ("gen1", BF16), ("gen1", GELU), ("gen1", RESID), ("gen1", PATCH),
                 ("gen1", QKV), ("8p", BF16), ("8p", GELU), ("8p", RESID), ("8p", PATCH), ("pp256", BF16), ("pp256", GELU), ("pp128", BF16)):
        assert need in epis, "no case runs %s with the %s epilogue" % (need[0], EPI_NAME[need[1]])
    # the skinny kernel's K edges: idle waves, a short last run, exactly R = 3, the first R = 4, 12 steps per wave
    ks = {c[2] for c in SKINNY_CASES}
    assert {64, 1088, 1152, 1216, 4352} <= ks
    per_wave = lambda K: -(-(K // 32) // SK_NW)
    assert per_wave(64) == 1 and 64 // 32 == 2                      # two waves work, ten idle
    assert per_wave(1088) == 3 and 1088 // 32 - 11 * 3 == 1         # the last wave's run is one step
    assert per_wave(1152) == 3 and 1152 // 32 == 36
    assert per_wave(1216) == 4 and -(-(1216 // 32) // 4) == 10      # waves 10 and 11 idle
    assert per_wave(4352) == 12 and 4352 // 32 - 11 * 12 == 4
    # mid prologue branches nk = 1, 2, 3, 4
    assert {c[2] // 64 for c in MID_CASES} >= {1, 2, 3, 4}
    # persistent kernels: an even and an odd number of K tiles
    assert {256 // 64 % 2, 320 // 64 % 2} == {0, 1}


def test_gelu_fit_error_is_what_the_kernel_states():
    """2.6e-5 (stated at gelu_coef) is part of the GELU bound: the polynomial in float64 against exact x Phi(x) over [-12, 12]."""
    x = np.linspace(-12, 12, 2_400_001)
    err = np.abs(gelu_kernel_formula(x, 0) - gelu_exact(x, 0)).max()
    print("erf flavour: largest |fit - x Phi(x)| on [-12, 12] = %.3e" % err)
    assert err <= GELU_FIT
    assert err > 1e-5            # the constant is not slack either
    err_t = np.abs(gelu_kernel_formula(x, 1) - gelu_exact(x, 1)).max()
    print("tanh flavour: largest |sigmoid form - tanh form| = %.3e" % err_t)
    assert err_t <= 1e-9
    src = _source("siglip_kernels.hip")
    for token in ("1.59501574f", "7.40113143e-02f", "-7.03036941e-04f", "1.5957691216f", "0.0713548163f", "float clamp = 50.0f"):
        assert token in src


def test_unit_roundoffs():
    """bf16 keeps 8 significant bits: round-to-nearest is off by up to 2^-8 |v|, and 2^-9 |v| is exceeded by rounding alone."""
    v = np.random.default_rng(1).uniform(1, 2, 100000).astype(np.float32)
    rel = np.abs(bf16_round(v).astype(np.float64) - v) / v
    assert 2.0 ** -9 < rel.max() <= U16
    relh = np.abs(f16_round(v).astype(np.float64) - v) / v
    assert 2.0 ** -12 < relh.max() <= UH
    assert SENT_BF16 < 0 and abs(SENT_BF16) < 1e-15 and abs(SENT_F16 + 0.02204) < 1e-5 and abs(SENT_F32) < 1e-15


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("epi,K,extra", [(BF16, 1152, ()), (GELU, 1152, ()), (PATCH, 640, (("tokens", 96),)), (RESID, 640, ()),
                                         (PART, 4352, (("ksplit", 4),))])
def test_bounds_are_not_vacuous(family, epi, K, extra):
    """The correctly rounded reference passes; the same array with 1 % of its elements one bf16 step further from the reference
    does not (integer family: is no longer equal)."""
    rows, N = 100, 128
    ref, bound, exact = reference(family, rows, N, K, epi, extra)
    store = {BF16: bf16_round, GELU: bf16_round, PATCH: f16_round}.get(epi, lambda v: v)
    good, bad, hit = perturbed(ref, store)
    assert worst(good, ref, bound)[0] <= 1.0
    if exact is not None:
        assert np.array_equal(good, exact) and not np.array_equal(bad, exact)
    ratio = ratios(bad, ref, bound)
    caught = (ratio[hit] > 1.0).mean()
    print("%s %s K %d: %.1f %% of the perturbed elements exceed the bound" % (EPI_NAME[epi], family, K, 100 * caught))
    assert ratio.max() > 1.0
    if epi == GELU:      # outputs near 0 have steps below the 2.6e-5 of the fit: counted where a step is at least 2^-10
        big = hit & (np.abs(ref) > 0.25)
        caught = (ratio[big] > 1.0).mean()
        print("    GELU, among outputs above 0.25: %.1f %%" % (100 * caught))
    assert caught > (0.99 if family == "int" else 0.25)


def test_hook_refuses_what_the_launchers_refuse(mse):
    from mse import ffi
    L = ffi.lib()
    assert L.mse_debug_siglip_gemm(None) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_gemm_fused(None) == -1 and "null argument" in ffi.last_error()
    ok = gemm_args(64, 128, 64, BF16, 1, ())
    assert L.mse_debug_siglip_gemm(C.byref(ok)) == 0 and ok.M == 256     # sizes only: nothing runs
    bad = [dict(rows=0), dict(N=32), dict(N=192), dict(K=32), dict(K=96), dict(skinny=5), dict(flags=8), dict(epi=5), dict(epi=7),
           dict(flags=2, n_valid=0), dict(flags=2, n_valid=129), dict(rows=1 << 20, K=1 << 10), dict(epi=PATCH, tokens=0),
           dict(epi=QKV, N=3 * D, heads=HEADS, dh=DH, tokens=64, rows=60), dict(epi=QKV, N=3 * D, heads=HEADS, dh=64, tokens=64),
           dict(epi=QKV, N=3 * D, heads=8, dh=DH, tokens=64), dict(epi=QKV, N=3 * D, heads=HEADS, dh=DH, tokens=32),
           dict(epi=PART, ksplit=4), dict(epi=PART, K=4352, ksplit=3), dict(epi=PART, K=4352, ksplit=4, rows=769),
           dict(epi=PART, K=1152, N=1152, ksplit=3, rows=65)]
    for change in bad:
        a = gemm_args(64, 128, 64, BF16, 1, ())
        for k, v in change.items():
            setattr(a, k, v)
        assert L.mse_debug_siglip_gemm(C.byref(a)) == -1 and "debug siglip gemm" in ffi.last_error(), change
    f = ffi.DebugSiglipGemmFusedArgs()
    f.rows, f.N, f.K, f.epi, f.eps = 256, 4352, 1152, GELU, 1e-6
    assert L.mse_debug_siglip_gemm_fused(C.byref(f)) == 0 and f.M == 256
    for change in (dict(K=192), dict(K=2112), dict(N=4480), dict(rows=100), dict(eps=0.0), dict(epi=BF16), dict(flags=4),
                   dict(epi=QKV), dict(epi=QKV, N=3 * D, heads=HEADS, dh=DH, tokens=64, K=1088),
                   dict(epi=RESID_LN, N=1280, n_valid=1100), dict(epi=RESID_LN, N=1536, n_valid=1152)):
        f = ffi.DebugSiglipGemmFusedArgs()
        f.rows, f.N, f.K, f.epi, f.eps = 256, 4352, 1152, GELU, 1e-6
        for k, v in change.items():
            setattr(f, k, v)
        assert L.mse_debug_siglip_gemm_fused(C.byref(f)) == -1 and "debug siglip gemm fused" in ffi.last_error(), change


def test_hook_comment_states_the_padding_contract():
    """The tests below hold the kernels to this text (check_padding, the QKV test); it must not drift from them silently."""
    src = " ".join(_source("siglip_api.hip").replace("//", " ").split())
    for sentence in (
            "rows rows .. rows rounded up to the tile height (64, 64, 128) are ZEROED, rows above keep what they held",
            "First-generation and non-persistent ping-pong kernels (K < 256, or the GELU remainder): rows rows .. M are ZEROED",
            "stores are unconditional -- rows rows .. M are OVERWRITTEN with bias + x_pad . w, finite when x's padding rows are finite",
            "RESID / PATCH every kernel skips rows >= rows (mok / m < m_valid): the padding rows keep what they held",
            "The persistent kernels (K >= 256) scatter EVERY row below M",
            "Columns dh .. of a q / K row, Vt's row-sum row dh and the rows above it are never written",
            "every slab is written up to rows rounded up to the tile height (64; 128 above SPLIT_T128_ROWS rows)",
            "every row below M is computed and stored like a real one"):
        assert sentence in src, sentence


# ---------------------------------------------------------------------------------------------------------
# GPU: the plain launches
# ---------------------------------------------------------------------------------------------------------
def families_of(case):
    rows, N, K, epi, skinny, extra = case
    if rows * N * K > 2 ** 31:
        return ["int", "gauss"]
    return ["int", "gauss", "heavy"]


def check_values(case, family, got_rows, what):
    """got_rows: the real rows of the output, shaped like reference()'s arrays."""
    rows, N, K, epi, skinny, extra = case
    ref, bound, exact = reference(family, rows, N, K, epi, extra)
    ratio, where = worst(got_rows, ref, bound)
    print("%s %-5s largest |got - ref| / bound %.3f; %s" % (what, family, ratio, where))
    assert np.isfinite(got_rows).all(), what
    if exact is not None:
        assert_same_bits(got_rows, exact, what + " (integer family: must be the correctly rounded exact value)")
    assert ratio <= 1.0, what + ": " + where
    return ratio


@pytest.mark.gpu
def test_hook_rounds_as_numpy_does(gpu):
    """x = identity reads w's rounding back through the BF16 epilogue (and w = identity x's), ties and odd mantissas included."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((128, 64)).astype(np.float32)
    u = v.view(np.uint32)
    u[0, :] = (u[0, :] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)       # exact ties
    u[1, :] = (u[1, :] & np.uint32(0xFFFE0000)) | np.uint32(0x18000)      # ties above an odd mantissa
    u[2, :] = (u[2, :] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
    eye = np.eye(64, dtype=np.float32)
    zero = np.zeros(128, np.float32)
    case = _c(64, 128, 64, BF16, 1)
    got = run_gemm(case, eye, v, zero, {})["out"][:64]
    assert_same_bits(got, bf16_round(v).T.copy(), "w rounding")
    w_eye = np.zeros((128, 64), np.float32)
    w_eye[:64] = eye
    got = run_gemm(case, v[:64], w_eye, zero, {})["out"][:64, :64]
    assert_same_bits(got.copy(), bf16_round(v[:64]), "x rounding")


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN_CASES, ids=case_id)
def test_gemm_against_float64(gpu, case):
    rows, N, K, epi, skinny, extra = case
    plan = dispatch(epi, rows, N, K, skinny)
    what = case_id(case) + " [" + " + ".join(p[0] for p in plan) + "]"
    side = not skinny and len(plan) > 1
    n_valid = N - 8
    for family in families_of(case):
        x, w, bias, aux = operands(family, rows, N, K, epi, extra)
        clean = run_gemm(case, x, w, bias, aux)
        a = clean["args"]
        dirty = run_gemm(case, x, w, bias, aux, flags=1 if epi == QKV else 3, n_valid=n_valid)
        if epi == QKV:
            ref, bound, exact = reference(family, rows, N, K, epi, extra)
            overwritten = np.zeros(3 * D, bool)     # columns whose kernel stores rows rows .. M unconditionally
            for kernel, c0, c1, mode in plan:
                overwritten[c0:c1] = mode == "finite"
            check_qkv(clean, dirty, rows, ref, bound, exact, overwritten, "%s %-5s" % (what, family))
        elif epi == PART:
            got = clean["out"]
            ref, bound, exact = reference(family, rows, N, K, epi, extra)
            check_values(case, family, got[:, :rows], what)
            edge = round_up(rows, plan[0][3][1])
            assert np.isfinite(got).all() and (got[:, edge:] == SENT_F32).all(), what + ": slab rows above the tile edge were written"
            total = got[:, :rows].astype(np.float64).sum(0) + bias.astype(np.float64)
            whole = ref.sum(0) + bias.astype(np.float64)
            ratio, where = worst(total, whole, bound.sum(0) + 2.0 ** -23 * np.abs(whole))
            assert ratio <= 1.0, what + " slabs + bias: " + where
            assert_same_bits(dirty["out"][:, :rows, :n_valid].copy(), got[:, :rows, :n_valid].copy(), what + ": padding reached real elements")
        else:
            got = clean["out"]
            check_values(case, family, got[:rows], what)
            check_padding(case, got, what)
            check_padding(case, dirty["out"], what + " (garbage in the padding)", n_valid)
            assert_same_bits(dirty["out"][:rows, :n_valid].copy(), got[:rows, :n_valid].copy(), what + ": padding reached real elements")
        if side:
            beside = run_gemm(case, x, w, bias, aux, flags=4)
            for name in ("out", "q", "k", "vt"):
                if name in clean:
                    assert_same_bits(beside[name], clean[name], what + ": remainder on a side stream")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEAM_CASES, ids=case_id)
def test_persistent_kernel_across_tile_seams(gpu, case):
    """More than 2 x CU count tiles: some workgroup walks three tiles, two seams, with the next tile's operands in flight."""
    import torch
    rows, N, K, epi, skinny, extra = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (rows // 256) * (N // 256)
    assert tiles > 2 * cus, "%d tiles on %d CUs: no workgroup walks three tiles -- enlarge the case" % (tiles, cus)
    for family in ("int", "gauss"):
        x, w, bias, aux = operands(family, rows, N, K, BF16, extra)     # one set of operands for both epilogues
        res = run_gemm(case, x, w, bias, aux)
        assert res["args"].cu_count == cus
        # the reference for these operands
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        pre = x64 @ w64.T + bias.astype(np.float64)
        E = accumulation_bound(family, K, np.abs(x64), np.abs(w64), pre)
        if epi == BF16:
            ref, bound = pre, E + U16 * (np.abs(pre) + E)
            if family == "int":
                assert_same_bits(res["out"], bf16_round(pre.astype(np.float32)), case_id(case))
        else:
            ref = gelu_exact(pre, 0)
            B = 1.13 * E + GELU_FIT + 2.0 ** -20 * np.abs(pre)
            bound = B + U16 * (np.abs(ref) + B)
        ratio, where = worst(res["out"], ref, bound)
        print("%s %-5s %d tiles on %d CUs: largest |got - ref| / bound %.3f; %s" % (case_id(case), family, tiles, cus, ratio, where))
        assert ratio <= 1.0, where


# ---------------------------------------------------------------------------------------------------------
# the LayerNorm-fused launches (image tower): consumers QKV / GELU, producer RESID_LN
# ---------------------------------------------------------------------------------------------------------
EPS = 1e-6
FUSED_CONSUMER_CASES = [(256, 4352, GELU), (512, 4352, GELU), (256, 3 * D, QKV), (512, 3 * D, QKV), (736, 3 * D, QKV)]
FUSED_PRODUCER_CASES = [(256, 1152), (512, 1152), (256, 4352), (512, 4352), (248, 1152)]
ROW_KINDS = ["N(0, 1)", "two massive channels", "mean 50, spread 0.5", "constant"]     # row m of the Gaussian family is kind m % 4


def stats_depth(width):
    """Additions a value passes through in row_stats_kernel's sums: a quad (3), the lane's pieces (width / 256), six shuffles; + 1 for
    the division.  The error of a sum is at most depth * 2^-24 * sum |terms|, whatever the values."""
    return 3 + -(-width // 256) + 6 + 1


def fold_depth(K):
    """The same for fold_ln_weights_kernel's two sums: a thread's K / 256 terms, eight halvings of 256 partial sums, + 1 (bias)."""
    return -(-K // 256) + 8 + 1


def row_stats_reference(x):
    """float64 (mean, 1/std) of fp16 rows and the bounds on what row_stats_kernel may return:
         |mean^ - mean| <= dm = depth 2^-24 mean|x|
         |rstd^ / rstd - 1| <= dr = ((depth + 5) 2^-24 var + dm^2) / (2 (var + eps)) + 2^-22
    (d = x - mean^ and its square: three roundings; the sum: depth; / width and + eps: two; sum (x - mean^)^2 = sum (x - mean)^2 +
    width (mean^ - mean)^2 exactly; rsqrtf: 2^-22.)"""
    x = np.asarray(x, np.float64)
    depth = stats_depth(x.shape[1])
    mu, var = x.mean(1), x.var(1)
    r = 1.0 / np.sqrt(var + EPS)
    dm = depth * 2.0 ** -24 * np.abs(x).mean(1)
    dr = ((depth + 5) * 2.0 ** -24 * var + dm * dm) / (2 * (var + EPS)) + 2.0 ** -22
    return mu, r, dm, dr


@functools.lru_cache(maxsize=2)
def consumer_operands(family, rows, N):
    rng = np.random.default_rng([rows, N, len(family)])
    K = D
    if family == "int":
        x = rng.integers(-8, 9, (rows, K)).astype(np.float32)
        w = rng.integers(-8, 9, (N, K)).astype(np.float32)
        bias = rng.integers(-16, 17, N).astype(np.float32)
        gamma = rng.integers(1, 3, K).astype(np.float32)
        beta = rng.integers(-2, 3, K).astype(np.float32)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
        kind = np.arange(rows) % 4
        big = np.flatnonzero(kind == 1)
        x[big[:, None], [[5, 700]]] = (rng.uniform(2000, 11000, (len(big), 2)) * rng.choice([-1, 1], (len(big), 2))).astype(np.float32)
        x[kind == 2] = 50.0 + 0.5 * x[kind == 2]
        x[kind == 3] = rng.uniform(-3, 3, ((kind == 3).sum(), 1)).astype(np.float32)
        w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
        bias = (rng.standard_normal(N) * math.sqrt(0.1)).astype(np.float32)
        gamma = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    x, w = f16_round(x), bf16_round(w)
    for a in (x, w, bias, gamma, beta):
        a.setflags(write=False)
    return x, w, bias, gamma, beta


def folded_weights(w, gamma):
    """w' as fold_ln_weights_kernel forms it: the fp32 product of the bf16 weight and gamma, rounded to fp16 (nearest even)."""
    return (w.astype(np.float32) * gamma.astype(np.float32)[None, :]).astype(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=2)
def consumer_reference(family, rows, N):
    """What the fused consumers compute, in float64, and the bound on the kernel's pre-activation:
        out = rstd (sum_k x_k w'_k - mean c_n) + b'_n,   w' = folded_weights(),  c_n = sum_k w'_nk,  b'_n = b_n + sum_k w_nk beta_k
    -- LayerNorm then Linear over the fp16 weights the kernel multiplies, so the fold's rounding is in the reference, not in the
    bound.  With u = 2^-24, C = sum |w'|, dc = fold_depth u C, (dm, dr) of row_stats_reference:
        c_n, b'_n     rstd |mean| dc  +  fold_depth u (|b| + sum |w beta|) + u |b'|          the two fp32 sums of the fold
        statistics    rstd (|c_n| + dc) dm  +  1.01 |out - b'| dr                            mean^ and rstd^ through rstd (acc - mean c)
        accumulation  rstd 2 (K + 2) u (sum |x w'| + |mean| (|c_n| + dc) + |b'| / rstd)      it starts at b' / rstd^ - mean^ c_n
        + 2 u |out|                                                                          the last multiply"""
    x, w, bias, gamma, beta = consumer_operands(family, rows, N)
    K = D
    x64, w64, b64, be64 = x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), beta.astype(np.float64)
    mu, r, dm, dr = row_stats_reference(x)
    wf = folded_weights(w, gamma)
    bp = b64 + w64 @ be64
    lin = ((x64 - mu[:, None]) @ wf.T) * r[:, None]
    pre = lin + bp
    u = 2.0 ** -24
    C = np.abs(wf).sum(1)
    dc = fold_depth(K) * u * C
    c = np.abs(wf.sum(1)) + dc
    rr, amu = r[:, None], np.abs(mu)[:, None]
    fold = rr * amu * dc[None, :] + (fold_depth(K) * u * (np.abs(b64) + np.abs(w64) @ np.abs(be64)) + u * np.abs(bp))[None, :]
    stat = rr * c[None, :] * dm[:, None] + np.abs(lin) * (dr[:, None] * 1.01)
    acc = rr * 2 * (K + 2) * u * (np.abs(x64) @ np.abs(wf).T + amu * c[None, :] + np.abs(bp)[None, :] / rr)
    bound = fold + stat + acc + 2 * u * np.abs(pre)
    return pre, bound, (mu, r, dm, dr)


def consumer_output(epi, pre, pb):
    """(ref, bound) of the stored bf16 output from the pre-activation and its bound."""
    if epi == GELU:
        ref = gelu_exact(pre, 0)
        B = 1.13 * pb + GELU_FIT + 2.0 ** -20 * np.abs(pre)
        return ref, B + U16 * (np.abs(ref) + B)
    return pre, pb + U16 * (np.abs(pre) + pb)


@functools.lru_cache(maxsize=2)
def producer_operands(family, rows, K):
    n_valid, N = D, round_up(D, 256)
    rng = np.random.default_rng([rows, K, len(family), 7])
    if family == "int":
        # |pre| <= 12 * 8 * 2 + 8 <= 256: exact as the bf16 the branch is staged in; |x + pre| <= 2048: exact in fp16
        x = np.zeros((rows, K), np.float32)
        cols = np.argsort(rng.random((rows, K)), axis=1)[:, :12]
        x[np.arange(rows)[:, None], cols] = rng.integers(-8, 9, (rows, 12)).astype(np.float32)
        w = rng.integers(-2, 3, (N, K)).astype(np.float32)
        bias = rng.integers(-8, 9, N).astype(np.float32)
        xres = rng.integers(-1500, 1501, (rows, n_valid)).astype(np.float32)
    else:
        x = rng.standard_normal((rows, K)).astype(np.float32)
        w = (rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)
        bias = (rng.standard_normal(N) * math.sqrt(0.1)).astype(np.float32)
        xres = rng.standard_normal((rows, n_valid)).astype(np.float32)
        xres[1::4, [5, 700]] = (rng.uniform(2000, 11000, (len(xres[1::4]), 2)) * rng.choice([-1, 1], (len(xres[1::4]), 2))).astype(np.float32)
        xres[2::4] = 50.0 + 0.5 * xres[2::4]
    w[n_valid:] = 0
    x, w, xres = bf16_round(x), bf16_round(w), f16_round(xres)
    for a in (x, w, bias, xres):
        a.setflags(write=False)
    return x, w, bias, xres


def producer_reference(family, rows, K):
    """(ref, bound) of the updated fp16 residual.  The integer family is exact at every step: its bound is 0."""
    x, w, bias, xres = producer_operands(family, rows, K)
    x64, w64 = x.astype(np.float64), w[:D].astype(np.float64)
    pre = x64 @ w64.T + bias[:D].astype(np.float64)
    ref = xres.astype(np.float64) + pre
    if family == "int":
        assert np.abs(pre).max() <= 256 and np.abs(ref).max() <= 2048
        return ref, np.zeros_like(ref)
    E = accumulation_bound(family, K, np.abs(x64), np.abs(w64), pre)
    d = E + U16 * (np.abs(pre) + E)                 # the branch is staged as bf16
    return ref, d + 2.0 ** -24 * np.abs(ref) + UH * (np.abs(ref) + d)


def perturbed(ref, store, seed=5):
    """(good, bad, hit): the correctly rounded reference, and the same with 1 % of its elements (hit) one bf16 step further from the
    reference -- 2^(floor(log2 |v|) - 7) at the element's own exponent."""
    good = store(ref.astype(np.float32))
    hit = np.random.default_rng(seed).random(ref.shape) < 0.01
    step = np.ldexp(1.0, np.frexp(np.abs(good))[1] - 8)
    bad = np.where(hit, good + np.where(good >= ref, step, -step).astype(np.float32), good).astype(np.float32)
    return good, bad, hit


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("epi", [QKV, GELU], ids=["QKV", "GELU"])
def test_fused_consumer_bound_against_one_bf16_step(family, epi):
    """CPU only.  The correctly rounded reference passes; with 1 % of its elements one bf16 step further away it does not.  How much of
    the perturbation a row's bound catches depends on what the row holds: the accumulation term is by LENGTH (2 K 2^-24 sum |x w'|, as for
    every GEMM here) and sum |x w'| grows with the row's mean while a bf16 step of the output does not.  Asserted where the derivation
    says the bound must bite -- integer rows (a step of at least 1 against about 0.9 + 2^-8 |out|), N(0, 1) rows (as the plain GEMM at
    K = 1152) and rows with massive channels (rstd of 1 / 300 shrinks every term) -- and reported, NOT claimed, for rows of mean 50 and
    constant rows, where the bound is of the order of the output: there the GPU test holds the kernel to its statistics, to finite
    values and to padding independence only."""
    rows, N = 256, (3 * D if epi == QKV else 4352)
    pre, pb, _ = consumer_reference(family, rows, N)
    ref, bound = consumer_output(epi, pre, pb)
    good, bad, hit = perturbed(ref, bf16_round)
    assert worst(good, ref, bound)[0] <= 1.0
    over = ratios(bad, ref, bound) > 1.0
    big = np.abs(ref) > 0.25          # (GELU: outputs near 0 have steps below the 2.6e-5 of the fit)
    if family == "int":
        caught = over[hit & big].mean()
        print("fused %s int: %.1f %% of the perturbed elements exceed the bound" % (EPI_NAME[epi], 100 * caught))
        assert caught > 0.25
        return
    kind = (np.arange(rows) % 4)[:, None] + np.zeros_like(ref, int)
    caught = [over[hit & big & (kind == k)].mean() for k in range(4)]
    for k in range(4):
        print("fused %s gauss, rows of kind '%s': median bound %.3g, %.1f %% of the perturbed elements exceed it" %
              (EPI_NAME[epi], ROW_KINDS[k], np.median(bound[kind == k]), 100 * caught[k]))
    assert caught[0] > 0.25 and caught[1] > 0.9


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("K", [1152, 4352])
def test_fused_producer_bound_against_one_bf16_step(family, K):
    """CPU only, as above, for the RESID_LN residual (an fp16 store).  Integer family: exact, every perturbed element is caught.
    Gaussian: rows of mean 50 (a bf16 step of 0.25) are always caught; rows of N(0, 1) as the plain GEMM of the same K -- at K = 4352
    E alone, 2 K 2^-24 S = 0.02, is above a bf16 step of a unit output, so nothing is claimed for them there (reported only)."""
    rows = 256
    ref, bound = producer_reference(family, rows, K)
    good, bad, hit = perturbed(ref, f16_round)
    assert worst(good, ref, bound)[0] <= 1.0
    over = ratios(bad, ref, bound) > 1.0
    if family == "int":
        assert over[hit].mean() > 0.99
        return
    kind = (np.arange(rows) % 4)[:, None] + np.zeros_like(ref, int)
    unit, mean50 = over[hit & (kind == 0)].mean(), over[hit & (kind == 2)].mean()
    print("RESID_LN gauss K %d: perturbed elements that exceed the bound: N(0, 1) rows %.1f %%, rows of mean 50 %.1f %%" % (K, 100 * unit, 100 * mean50))
    assert mean50 > 0.99 and (K > 1152 or unit > 0.25)


def run_fused(epi, rows, N, K, x, w, bias, gamma=None, beta=None, xres=None, flags=0, n_valid=0, tokens=0, gelu_tanh=0):
    from mse import ffi
    a = ffi.DebugSiglipGemmFusedArgs()
    a.rows, a.N, a.K, a.epi, a.gelu_tanh, a.flags, a.n_valid, a.eps = rows, N, K, epi, gelu_tanh, flags, n_valid, EPS
    if epi == QKV:
        a.heads, a.dh, a.tokens = HEADS, DH, tokens
    L = ffi.lib()
    ffi.check(L.mse_debug_siglip_gemm_fused(C.byref(a)), "mse_debug_siglip_gemm_fused (sizes)")
    keep = {n: np.ascontiguousarray(v, np.float32) for n, v in dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, xres=xres).items() if v is not None}
    for n, v in keep.items():
        setattr(a, n, _p(v))
    res = {"stats": np.full((a.M, 2), np.nan, np.float32)}
    a.stats = _p(res["stats"])
    if epi == QKV:
        mats = a.n_seq * HEADS
        res["q"] = np.full((mats, a.n_pad, a.dh_pad), np.nan, np.float32)
        res["k"] = np.full((mats, a.n_pad, a.kdh_pad), np.nan, np.float32)
        res["vt"] = np.full((mats, a.dv_pad, a.n_pad), np.nan, np.float32)
        a.q, a.k, a.vt = _p(res["q"]), _p(res["k"]), _p(res["vt"])
    else:
        res["out"] = np.full((a.M, n_valid if epi == RESID_LN else N), np.nan, np.float32)
        a.out = _p(res["out"])
    ffi.check(L.mse_debug_siglip_gemm_fused(C.byref(a)), "mse_debug_siglip_gemm_fused %s rows %d" % (EPI_NAME[epi], rows))
    res["args"] = a
    return res


def check_stats(got, ref, rows, what):
    mu, r, dm, dr = ref
    em = np.abs(got[:rows, 0].astype(np.float64) - mu) / (dm + 2.0 ** -24 * np.abs(mu) + 1e-300)
    er = np.abs(got[:rows, 1].astype(np.float64) / r - 1.0) / dr
    print("%s statistics: largest |mean^ - mean| / bound %.3f (row %d), |rstd^ / rstd - 1| / bound %.3f (row %d)" %
          (what, em.max(), em.argmax(), er.max(), er.argmax()))
    assert np.isfinite(got).all()
    assert em.max() <= 1.0 and er.max() <= 1.0, what


@pytest.mark.gpu
@pytest.mark.parametrize("rows,N,epi", FUSED_CONSUMER_CASES, ids=lambda v: str(v))
def test_fused_consumers_against_float64(gpu, rows, N, epi):
    tokens = 736 if rows == 736 else 64
    what = "fused %s rows %d" % (EPI_NAME[epi], rows)
    for family in ("int", "gauss"):
        x, w, bias, gamma, beta = consumer_operands(family, rows, N)
        pre, pb, stats_ref = consumer_reference(family, rows, N)
        ref, bound = consumer_output(epi, pre, pb)
        clean = run_fused(epi, rows, N, D, x, w, bias, gamma, beta, tokens=tokens)
        dirty = run_fused(epi, rows, N, D, x, w, bias, gamma, beta, tokens=tokens, flags=1)
        check_stats(clean["stats"], stats_ref, rows, what + " " + family)
        assert np.isfinite(dirty["stats"]).all()
        assert_same_bits(dirty["stats"][:rows].copy(), clean["stats"][:rows].copy(), what + ": padding reached the statistics of real rows")
        if epi == QKV:
            check_qkv(clean, dirty, rows, ref, bound, None, np.ones(3 * D, bool), "%s %-5s" % (what, family))
            continue
        got = clean["out"]
        ratio = ratios(got[:rows], ref, bound)
        print("%s %-5s largest |got - ref| / bound %.3f; %s" % (what, family, ratio.max(), worst(got[:rows], ref, bound)[1]))
        if family == "gauss":
            print("    by row kind: " + ", ".join("%s %.3f" % (ROW_KINDS[k], ratio[k::4].max()) for k in range(4)))
        assert np.isfinite(got).all() and np.isfinite(dirty["out"]).all() and ratio.max() <= 1.0, what
        assert_same_bits(dirty["out"][:rows].copy(), got[:rows].copy(), what + ": padding reached real rows")


@pytest.mark.gpu
@pytest.mark.parametrize("rows,K", FUSED_PRODUCER_CASES, ids=lambda v: str(v))
def test_fused_producer_against_float64(gpu, rows, K):
    n_valid, N = D, round_up(D, 256)
    what = "fused RESID_LN rows %d K %d" % (rows, K)
    for family in ("int", "gauss"):
        x, w, bias, xres = producer_operands(family, rows, K)
        clean = run_fused(RESID_LN, rows, N, K, x, w, bias, xres=xres, n_valid=n_valid)
        dirty = run_fused(RESID_LN, rows, N, K, x, w, bias, xres=xres, n_valid=n_valid, flags=3)
        ref, bound = producer_reference(family, rows, K)
        got = clean["out"]
        ratio, where = worst(got[:rows], ref, bound)
        print("%s %-5s largest |got - ref| / bound %.3f; %s" % (what, family, ratio, where))
        assert np.isfinite(got).all() and np.isfinite(clean["stats"]).all(), what
        if family == "int":
            assert_same_bits(got[:rows].copy(), ref.astype(np.float32), what + " (integer family: must be exact)")
        assert ratio <= 1.0, where
        # the statistics describe the sums BEFORE their fp16 store: against float64 over the stored row they may differ by that
        # rounding (2^-11 |v| per element: 2^-11 mean|v| on the mean, 2^-11 rms(v) / std on 1/std) on top of the fp32 terms
        v = got[:rows].astype(np.float64)
        mu, r, dm, dr = row_stats_reference(v)
        depth = 3 + 3 + n_valid // 64 + 2          # a lane's eight, sum8, the groups in ln_stats_finalize_kernel, the divisions
        dm = depth * 2.0 ** -24 * np.abs(v).mean(1) + (0.0 if family == "int" else UH * np.abs(v).mean(1))
        var = v.var(1)
        dr = ((depth + 8) * 2.0 ** -24 * var + dm * dm) / (2 * (var + EPS)) + 2.0 ** -22
        dr = dr + (0.0 if family == "int" else UH * np.sqrt((v * v).mean(1)) * r * 1.01)
        check_stats(clean["stats"], (mu, r, dm, dr), rows, what + " " + family)
        assert_same_bits(dirty["out"][:rows].copy(), got[:rows].copy(), what + ": padding reached real rows")
        assert_same_bits(dirty["stats"][:rows].copy(), clean["stats"][:rows].copy(), what + ": padding reached the statistics of real rows")


@pytest.mark.gpu
def test_fused_hook_rounds_as_numpy_does(gpu):
    """Zero weights and bias: the producer returns fp16(xres) itself, ties included; its statistics are those of that row."""
    rng = np.random.default_rng(11)
    xres = rng.standard_normal((256, D)).astype(np.float32)
    u = xres.view(np.uint32)
    u[0, :] = (u[0, :] & np.uint32(0xFFFFE000)) | np.uint32(0x1000)       # exact fp16 ties
    u[1, :] = (u[1, :] & np.uint32(0xFFFFC000)) | np.uint32(0x3000)       # ties above an odd mantissa
    N = round_up(D, 256)
    res = run_fused(RESID_LN, 256, N, 256, np.zeros((256, 256), np.float32), np.zeros((N, 256), np.float32), np.zeros(N, np.float32),
                    xres=xres, n_valid=D)
    assert_same_bits(res["out"], f16_round(xres), "fp16 rounding of the residual")
