"""The SigLIP row kernels, each alone: layernorm_kernel / layernorm_wg_kernel (fp32 and fp16 x), patchify_kernel / patchify8_kernel,
rgb8_to_nchw_f16_kernel, bmp24_to_nchw_f16_kernel, embed_tokens_kernel, f32_to_bf16_pad_kernel, small_linear_kernel, l2norm_kernel and
vt_ones_row_kernel -- everything in siglip_kernels.hip that the GEMM and attention files do not reach and that test_siglip.py sees only
at the end of a whole forward pass, at a cosine-level tolerance.

Everything goes through the mse_debug_siglip_<launcher> hooks (siglip_api.hip): ONE call of the launcher the towers use, every
destination between guard bands and filled with bytes 0xA5, returned whole.  kernel_of() restates which kernel a launcher picks (a
CPU test pins that to the source, another shows that every kernel has a case).  The reference is numpy over the operands as the hook
rounds them (bf16_round / f16_round restate that).

Exact kernels (the decoders, patchify, embed_tokens, f32_to_bf16_pad, vt_ones_row, LayerNorm's write-back of x, a constant LayerNorm row,
l2norm without normalisation and of a basis vector, small_linear on integers) are compared bit for bit: the library is built with
-ffp-contract=off -fno-fast-math, so numpy float32 restates them.

Bounds of the rest, per element, from the operands and the float64 reference only, u = 2^-24:
  LayerNorm     v = x + delta exact in float64; L = 40 bounds the fp32 additions an element's sums pass through (8 x 4 + 6 in
                layernorm_kernel at width 2048, 2 x 4 + 6 + 3 in layernorm_wg_kernel: test_addition_counts_match_the_source);
                n_a = additions that form v (0 none, 1 bf16 delta, n_parts + 1 parts); a_i = sum of |terms| of v_i
                    e_v   = n_a u a_i
                    e_mu  = (L + 1) u mean|v| + mean(e_v)
                    d     = v - mu;  s2 = var + eps;  r = s2^-1/2
                    e_d   = e_v + e_mu + u |d|
                    e_var = mean(2 |d| e_d + e_d^2) + (L + 3) u (var + mean(e_d^2)) + u s2
                    e_r   = 1.01 * 0.5 * e_var / s2 + 2^-21          (rsqrtf, the add of eps, the divide)
                    E     = |gamma| r (e_d + |d| e_r) + 3 u |gamma d r| + u |ref|
                fp32 output |got - ref| <= E; bf16 output E + 2^-8 (|ref| + E)
  small_linear  (ceil(K / 64) + 8) u S + u |ref|,  S = sum |x_k w_k| + |bias|, w as bf16
  l2norm        fp32 |ref| (1.01 * 0.5 * (ceil(W / 64) + 7) u + 3 u); fp16 adds 2^-11 |ref| + 2^-25
launch_patchify refuses k_pad < C P P and an image below one patch, NOT H % P or W % P: the grid is H / P x W / P as for the stride-P
convolution, no read leaves the image, and the shipped geometry (384 pixels, 14-pixel patches) leaves 6 pixels over -- the 34 x 48 case
pins that they are ignored.
None of these is a measured number.  The largest |got - ref| / bound measured per kernel and family is kept in DESIGN 3.4.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT

U = 2.0 ** -24
U16 = 2.0 ** -8        # unit roundoff of bf16 (8 significant bits)
UH = 2.0 ** -11        # of fp16 (11)
EPS = 1e-6
L_ADDS = 40
CSRC = os.path.join(ROOT, "meme-search-engine_amd", "csrc")

SENT_BF16 = np.array([0xA5A5 << 16], np.uint32).view(np.float32)[0]
SENT_F16 = np.array([0xA5A5], np.uint16).view(np.float16).astype(np.float32)[0]
SENT_F32 = np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0]


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def f16_round(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def assert_same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, "%s: shapes %s and %s" % (what, a.shape, b.shape)
    d = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert d.size == 0, "%s: %d elements differ, the first at %s: %r against %r" % (what, len(d), d[0].tolist(), a[tuple(d[0])], b[tuple(d[0])])


def ratios(got, ref, bound):
    diff = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0, 0.0, diff / bound)
    return np.where(np.isfinite(ratio), ratio, np.inf)


def worst(got, ref, bound):
    ratio = ratios(got, ref, bound)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), "worst at %s: got %.9g, reference %.9g, bound %.3g" % (list(map(int, i)), np.asarray(got)[i], ref[i], bound[i])


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pu8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------
# LayerNorm: input families, float64 reference and bound, float32 restatement of the kernels' own summation order
# ---------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "massive", "offset", "eps", "constant")
WIDTHS = (4, 256, 260, 1024, 1028, 1152, 2048)
ROWS = (1, 4, 5, 7)
DELTAS = (("none", 0), ("bf16", 0), ("parts", 1), ("parts", 2), ("parts", 4))
OUTS = ("bf16", "f32", "both")


def family_row(family, width, rng):
    """(x, total delta) of one row, float32.  The delta of the constant family is zero and of the eps-dominated one as small as x."""
    if family == "constant":
        return np.full(width, 3.0, np.float32), np.zeros(width, np.float32)
    if family == "eps":
        return (1e-3 * rng.standard_normal(width)).astype(np.float32), (1e-3 * rng.standard_normal(width)).astype(np.float32)
    if family == "offset":
        return (100.0 + rng.uniform(-0.5, 0.5, width)).astype(np.float32), (0.1 * rng.standard_normal(width)).astype(np.float32)
    x = rng.standard_normal(width).astype(np.float32)
    if family == "massive":     # as test_engine_with_massive_activation_channels: two channels of 300 and -180 among unit ones
        a, b = rng.choice(width, 2, replace=False)
        x[a], x[b] = 300.0, -180.0
    return x, (0.5 * rng.standard_normal(width)).astype(np.float32)


def ln_operands(width, rows, x_is_f16, delta, n_parts, shift, seed=0):
    """One launch: row i comes from family FAMILIES[(i + shift) % 5].  Returns x [rows][width] as the hook rounds it, `terms` (the
    float32 arrays added to x, in the kernel's order: the bf16 delta, or the parts then the bias), gamma, beta and the family names."""
    rng = np.random.default_rng([width, rows, x_is_f16, len(delta), n_parts, shift, seed])
    fams = [FAMILIES[(i + shift) % len(FAMILIES)] for i in range(rows)]
    pairs = [family_row(f, width, rng) for f in fams]
    x = np.stack([p[0] for p in pairs])
    x = f16_round(x) if x_is_f16 else x
    total = np.stack([p[1] for p in pairs])
    gamma = (1.0 + 0.2 * rng.standard_normal(width)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(width)).astype(np.float32)
    terms = []
    if delta == "bf16":
        terms = [bf16_round(total)]
    elif delta == "parts":
        bias = (0.1 * rng.standard_normal(width)).astype(np.float32)
        parts = [(0.3 * rng.standard_normal((rows, width))).astype(np.float32) for _ in range(n_parts - 1)]
        for i, f in enumerate(fams):       # the small families: the slabs before the last are small too (constant: zero)
            for q in parts:
                q[i] *= {"constant": 0.0, "eps": 1e-3}.get(f, 1.0)
        last = total - bias
        for q in parts:
            last = last - q
        terms = parts + [last.astype(np.float32), bias]
    for a in (x, gamma, beta, *terms):
        a.setflags(write=False)
    return x, terms, gamma, beta, fams


def ln_v32(x, terms, delta):
    """The kernels' own v: x + delta, or x + ((((p0 + p1) + ...) + p_last) + bias), in float32."""
    if delta == "none":
        return x
    if delta == "bf16":
        return x + terms[0]
    d = terms[0]
    for q in terms[1:-1]:
        d = d + q
    return x + (d + terms[-1][None, :])


def ln_reference(x, terms, delta, gamma, beta, eps=EPS):
    """(ref, E) in float64 from the exact v = x + sum(terms)."""
    x64 = x.astype(np.float64)
    t64 = [np.broadcast_to(t.astype(np.float64), x.shape) for t in terms]
    v = x64 + sum(t64) if t64 else x64
    a = np.abs(x64) + sum(np.abs(t) for t in t64) if t64 else np.abs(x64)
    n_a = {"none": 0, "bf16": 1}.get(delta, len(terms))      # parts: n_parts + 1 (the slabs among themselves, the bias, x)
    mean = lambda z: z.mean(axis=1, keepdims=True)
    g = np.abs(gamma.astype(np.float64))
    e_v = n_a * U * a
    mu = mean(v)
    e_mu = (L_ADDS + 1) * U * mean(np.abs(v)) + mean(e_v)
    d = v - mu
    var = mean(d * d)
    s2 = var + eps
    r = s2 ** -0.5
    e_d = e_v + e_mu + U * np.abs(d)
    e_var = mean(2 * np.abs(d) * e_d + e_d ** 2) + (L_ADDS + 3) * U * (var + mean(e_d ** 2)) + U * s2
    e_r = 1.01 * 0.5 * e_var / s2 + 2.0 ** -21
    ref = gamma.astype(np.float64) * d * r + beta.astype(np.float64)
    E = g * r * (e_d + np.abs(d) * e_r) + 3 * U * np.abs(gamma * d * r) + U * np.abs(ref)
    return ref, E


def bf16_bound(ref, E):
    return E + U16 * (np.abs(ref) + E)


def restate_layernorm(v, gamma, beta, wg=0, eps=EPS, variant=None):
    """layernorm_kernel (wg = 0) / layernorm_wg_kernel (wg = 1) in numpy float32, in the kernels' own summation order: a lane adds its
    4-element pieces ((x + y) + z) + w, piece after piece; the 64 lanes meet in a butterfly (offsets 32 .. 1); the workgroup
    kernel then adds its four waves ((w0 + w1) + w2) + w3.  Returns (out_f32, out_bf16).
    variant: a deliberately wrong kernel -- "width-1" (divisor of the variance), "dropped-piece" (the last 4 columns missing from
    the sums), "f16-stats" (statistics and normalisation from the fp16-rounded v), "bf16-step" (the bf16 result one step off)."""
    f32 = np.float32
    rows, width = v.shape
    J, NW = (2, 4) if wg else (8, 1)
    cap = J * NW * 256
    if variant == "f16-stats":
        v = f16_round(v)
    vp = np.zeros((rows, cap), f32)
    vp[:, :width] = v
    mask = np.zeros(cap, bool)
    mask[:width - 4 if variant == "dropped-piece" else width] = True
    vp = vp.reshape(rows, J, NW, 64, 4)
    mask = mask.reshape(1, J, NW, 64, 4)
    lanes = np.arange(64)

    def total(pieces):      # [rows][J][NW][64][4] -> [rows][1]
        s = np.zeros((rows, NW, 64), f32)
        for j in range(J):
            q = pieces[:, j]
            s = s + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, :, lanes ^ o]
        s = s[:, :, 0]
        t = s[:, 0]
        for w in range(1, NW):
            t = t + s[:, w]
        return t.reshape(rows, 1, 1, 1, 1)

    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total(np.where(mask, vp, f32(0))) / f32(width)
        d = np.where(mask, vp - mean, f32(0))
        ss = total(d * d)
        div = f32(width - 1) if variant == "width-1" else f32(width)
        rstd = (1.0 / np.sqrt((ss / div + f32(eps)).astype(np.float64))).astype(f32)
        y = ((vp - mean) * rstd).reshape(rows, cap)[:, :width] * gamma + beta
    y = y.astype(f32)
    yb = bf16_round(y)
    if variant == "bf16-step":
        yb = (yb.view(np.uint32) + np.uint32(0x10000)).view(f32)
    return y, yb


# the LayerNorm launches: (width, rows, x_is_f16, wg, delta, n_parts, outs, ldx, ldd, ldp, ldo, shift)
def _ln(width, rows, x_is_f16, wg, delta, n_parts, outs, ldx=None, ldd=None, ldp=None, ldo=None, shift=0):
    return (width, rows, x_is_f16, wg, delta, n_parts, outs, ldx or width + 8, ldd or width + 4, ldp or width + 12, ldo or width + 16, shift)


def ln_id(c):
    width, rows, x_is_f16, wg, delta, n_parts, outs, ldx, ldd, ldp, ldo, shift = c
    return "w%d-r%d-%s-wg%d-%s%s-%s-ldx%d" % (width, rows, "f16" if x_is_f16 else "f32", wg, delta, n_parts or "", outs, ldx)


def _ln_grid():
    """Every (width, kernel, x type, delta form); rows, outputs and the family of row 0 rotate so that each kernel and x type meets
    every row count, every output set and every family at every width (test_every_kernel_has_a_case checks the rotation)."""
    out, i = [], 0
    for width in WIDTHS:
        for wg in (0, 1):
            for x_is_f16 in (1, 0):
                for delta, n_parts in DELTAS:
                    out.append(_ln(width, ROWS[i % 4], x_is_f16, wg, delta, n_parts, OUTS[(i // 4 + i) % 3], shift=i))
                    i += 1
                i += 1       # 5 delta forms, then skip one: the rotation of rows does not lock to the delta form
    return out


LN_GRID = _ln_grid()
# the towers' forms at width 1152 (siglip_encoder.hip, siglip_api.hip, siglip_text_api.hip)
LN_TOWER = (
    [_ln(1152, 7, 1, wg, delta, n_parts, "bf16", ldx=1152, ldd=1152, ldp=1152, ldo=1152, shift=2) for wg in (0, 1) for delta, n_parts in DELTAS] +
    [_ln(1152, 5, 0, 1, "none", 0, "bf16", ldx=1152, ldo=1152, shift=1),            # pooled rows (MAP head): fp32 x, no delta
     _ln(1152, 5, 1, 1, "none", 0, "f32", ldx=64 * 1152, ldo=1152, shift=3),        # text final: the last token of each text
     _ln(1152, 4, 1, 1, "bf16", 0, "f32", ldx=64 * 1152, ldd=1152, ldo=1152, shift=4)])
LN_CASES = LN_GRID + LN_TOWER


def run_layernorm(case, x, terms, gamma, beta, eps=EPS):
    from mse import ffi
    width, rows, x_is_f16, wg, delta, n_parts, outs, ldx, ldd, ldp, ldo, shift = case
    a = ffi.DebugSiglipLayernormArgs()
    a.rows, a.width, a.ldx, a.x_is_f16, a.ldo, a.wg, a.eps = rows, width, ldx, x_is_f16, ldo, wg, eps
    keep = [np.ascontiguousarray(v, np.float32) for v in (x, gamma, beta)]
    a.x, a.gamma, a.beta = (_p(v) for v in keep)
    if delta == "bf16":
        keep.append(np.ascontiguousarray(terms[0], np.float32))
        a.delta, a.ldd = _p(keep[-1]), ldd
    elif delta == "parts":
        keep.append(np.ascontiguousarray(np.stack(terms[:-1]), np.float32))
        keep.append(np.ascontiguousarray(terms[-1], np.float32))
        a.parts, a.bias, a.n_parts, a.part_rows, a.ldp = _p(keep[-2]), _p(keep[-1]), n_parts, rows + 3, ldp
    res = {"x": np.full((rows, ldx), np.nan, np.float32)}
    a.x_out = _p(res["x"])
    if outs in ("bf16", "both"):
        res["out"] = np.full((rows, ldo), np.nan, np.float32)
        a.out = _p(res["out"])
    if outs in ("f32", "both"):
        res["out_f32"] = np.full((rows, ldo), np.nan, np.float32)
        a.out_f32 = _p(res["out_f32"])
    ffi.check(ffi.lib().mse_debug_siglip_layernorm(C.byref(a)), "mse_debug_siglip_layernorm " + ln_id(case))
    return res


# ---------------------------------------------------------------------------------------------------------
# which kernel a launcher picks, restated from siglip_kernels.hip (test_kernel_selection_matches_the_source pins it)
# ---------------------------------------------------------------------------------------------------------
PATCHIFY_CASES = (        # (P, C, H, W, k_pad, B, tstride)
    (14, 3, 28, 42, 640, 2, 8),
    (4, 2, 8, 12, 40, 2, 6),
    (14, 6, 28, 42, 1184, 2, 8),
    (14, 3, 34, 48, 640, 2, 8))       # 6 pixels past the last whole patch each way, as the shipped 384 / 14: ignored
EMBED_WIDTHS = (8, 516, 1152)
PAD_CASES = ((3, 5, 7, 256, 8), (5, 1152, 1152, 256, 1152), (4104, 5, 7, 4104, 4096))     # rows, cols, ld_in, rows_pad, cols_pad
LINEAR_KS = (1, 64, 70, 1152)
LINEAR_SHAPES = ((1, 1152), (3, 5))      # (B, N)
L2_WIDTHS = (1, 64, 70, 1152)
VT_PADS = (32, 96)


def kernel_of(launcher, *a):
    if launcher == "layernorm":
        x_is_f16, wg = a
        return "%s<%s>" % ("layernorm_wg_kernel" if wg else "layernorm_kernel", "_Float16" if x_is_f16 else "float")
    if launcher == "patchify":
        P, k_pad, is_f16 = a
        return "%s<%s>" % ("patchify8_kernel" if P == 14 and k_pad % 8 == 0 and k_pad <= 1024 else "patchify_kernel", "_Float16" if is_f16 else "float")
    return {"rgb8": "rgb8_to_nchw_f16_kernel", "bmp24": "bmp24_to_nchw_f16_kernel", "embed_tokens": "embed_tokens_kernel",
            "f32_to_bf16_pad": "f32_to_bf16_pad_kernel", "small_linear": "small_linear_kernel", "l2norm": "l2norm_kernel",
            "vt_ones_row": "vt_ones_row_kernel"}[launcher]


REQUIRED_KERNELS = {"layernorm_kernel<float>", "layernorm_kernel<_Float16>", "layernorm_wg_kernel<float>", "layernorm_wg_kernel<_Float16>",
                    "patchify_kernel<float>", "patchify_kernel<_Float16>", "patchify8_kernel<float>", "patchify8_kernel<_Float16>",
                    "rgb8_to_nchw_f16_kernel", "bmp24_to_nchw_f16_kernel", "embed_tokens_kernel", "f32_to_bf16_pad_kernel",
                    "small_linear_kernel", "l2norm_kernel", "vt_ones_row_kernel"}


# ---------------------------------------------------------------------------------------------------------
# CPU-only checks
# ---------------------------------------------------------------------------------------------------------
def test_kernel_selection_matches_the_source():
    """kernel_of() restates the launchers; a changed condition must fail here instead of silently un-testing a kernel."""
    src = _source("siglip_kernels.hip")
    for line in (
            "if (P == 14 && k_pad % 8 == 0 && k_pad <= 1024 && (size_t)B * tstride < (1u << 31)) {",
            "hipLaunchKernelGGL((patchify8_kernel<_Float16, 14>), dim3(rows), dim3(128)",
            "if (wg) {   // few rows in the CALL: a workgroup per row",
            "hipLaunchKernelGGL(layernorm_wg_kernel<_Float16>, dim3((unsigned)rows), dim3(256)",
            "hipLaunchKernelGGL(layernorm_kernel<float>, dim3((unsigned)((rows + 3) / 4)), dim3(256)",
            "unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 65535);",
            "hipLaunchKernelGGL(small_linear_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256)",
            "hipLaunchKernelGGL(embed_tokens_kernel, dim3((unsigned)rows), dim3(128)",
            # the refusals the hooks repeat before they allocate
            'if (width % 4 || width > 2048) return fail("layernorm: width must be a multiple of 4, at most 2048");',
            'if (delta.parts && (delta.bf16 || delta.n_parts < 1 || !delta.bias || delta.ldp % 4)) return fail("layernorm: bad partial-sum delta");',
            'if (P <= 0 || H < P || W < P) return fail("patchify: the image must hold at least one patch");',
            'if (k_pad < C * P * P) return fail("patchify: k_pad is smaller than a patch (C * P * P)");',
            'if (D % 4) return fail("embed tokens: width must be a multiple of 4");',
            'if (dh != 72 || dv_pad != 80) return fail("attention: the row-sum row assumes dh 72, dv_pad 80");'):
        assert line in src, "siglip_kernels.hip changed: %r is gone -- update kernel_of() and the cases with it" % line
    # the dead activation / residual parameters of the small linear layer are gone
    for gone in ("gelu_erf", "float gelu_tanh(", "ldres", "int act"):
        assert gone not in src, gone
    for name in ("siglip.h", "siglip_api.hip", "siglip_text_api.hip"):
        assert "ldres" not in _source(name)


def test_every_kernel_has_a_case(capsys):
    reached = {}
    for c in LN_CASES:
        reached.setdefault(kernel_of("layernorm", c[2], c[3]), []).append(ln_id(c))
    for P, Cc, H, W, k_pad, B, ts in PATCHIFY_CASES:
        for is_f16 in (1, 0):
            reached.setdefault(kernel_of("patchify", P, k_pad, is_f16), []).append("P%d-C%d-k%d" % (P, Cc, k_pad))
    for name, cases in (("rgb8", [(2, 5, 7)]), ("bmp24", [7, 8]), ("embed_tokens", EMBED_WIDTHS), ("f32_to_bf16_pad", PAD_CASES),
                        ("small_linear", LINEAR_KS), ("l2norm", L2_WIDTHS), ("vt_ones_row", VT_PADS)):
        reached.setdefault(kernel_of(name), []).extend(map(str, cases))
    with capsys.disabled():
        for k in sorted(reached):
            print("\n%-28s %3d cases, e.g. %s" % (k, len(reached[k]), ", ".join(reached[k][:2])), end="")
        print()
    assert REQUIRED_KERNELS <= set(reached), "no case reaches %s" % sorted(REQUIRED_KERNELS - set(reached))
    assert set(WIDTHS) == {4, 256, 260, 1024, 1028, 1152, 2048} and set(ROWS) == {1, 4, 5, 7}
    assert {(d, n) for d, n in DELTAS} == {("none", 0), ("bf16", 0), ("parts", 1), ("parts", 2), ("parts", 4)}
    # each LayerNorm kernel meets every width x delta form, every row count, every output set, and every family at every width
    for wg in (0, 1):
        for f16 in (0, 1):
            mine = [c for c in LN_GRID if c[2] == f16 and c[3] == wg]
            assert {(c[0], c[4], c[5]) for c in mine} == {(w, d, n) for w in WIDTHS for d, n in DELTAS}
            assert {c[1] for c in mine} == set(ROWS) and {c[6] for c in mine} == set(OUTS)
            for w in WIDTHS:
                fams = {FAMILIES[(i + c[11]) % 5] for c in mine if c[0] == w for i in range(c[1])}
                assert fams == set(FAMILIES), (wg, f16, w, fams)
    assert all(c[7] > c[0] and c[8] > c[0] and c[9] > c[0] and c[10] > c[0] for c in LN_GRID)      # every leading dimension above the width
    # the ragged last workgroup of the wave-per-row kernel (4 waves): 1, 5 and 7 rows
    assert {r % 4 for r in ROWS} >= {0, 1, 3}
    # the towers' forms
    assert sum(1 for c in LN_TOWER if c[2] == 1 and c[7] == 1152 and c[6] == "bf16") == 2 * len(DELTAS)
    assert any(c[2] == 0 and c[3] == 1 and c[4] == "none" for c in LN_TOWER)
    assert any(c[7] == 64 * 1152 and c[6] == "f32" and c[3] == 1 for c in LN_TOWER)
    # patchify: gw != gh, padded token rows, the 1024-column limit of the fast kernel; small_linear: one lane, one full pass, a ragged one
    for P, Cc, H, W, k_pad, B, ts in PATCHIFY_CASES:
        assert H // P != W // P and ts >= (H // P) * (W // P) and k_pad >= Cc * P * P
    assert PATCHIFY_CASES[0][6] > 6 and PATCHIFY_CASES[2][4] > 1024 and PATCHIFY_CASES[3][2] % 14 == 6 == 384 % 14
    assert 516 == 128 * 4 + 4 and PAD_CASES[2][3] * PAD_CASES[2][4] > 65535 * 256
    assert (3 * 5 + 3) // 4 * 4 > 3 * 5                       # 15 waves: the last workgroup is ragged


def test_addition_counts_match_the_source():
    """L = 40 in the bound: the fp32 additions an element's row sum passes through, counted in the source."""
    src = _source("siglip_kernels.hip")
    wave = src[src.index("void layernorm_kernel("):src.index("void layernorm_wg_kernel(")]
    wg = src[src.index("void layernorm_wg_kernel("):src.index("void ln_stats_finalize_kernel(")]
    assert "float4 v[8];" in wave and wave.count("for (int j = 0; j < 8; j++)") == 3
    assert "s += v[j].x + v[j].y + v[j].z + v[j].w;" in wave and "ss += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;" in wave
    assert wave.count("for (int o = 32; o >= 1; o >>= 1)") == 2 and "if (width % 4 || width > 2048)" in src
    assert "float4 v[2], gm[2], bt[2];" in wg and wg.count("for (int j = 0; j < 2; j++)") == 3 and "const int c = tid * 4 + j * 1024;" in wg
    assert "s += v[j].x + v[j].y + v[j].z + v[j].w;" in wg and wg.count("for (int o = 32; o >= 1; o >>= 1)") == 2
    assert "(((s_part[0][0] + s_part[0][1]) + s_part[0][2]) + s_part[0][3]) / (float)width" in wg
    assert "(((s_part[1][0] + s_part[1][1]) + s_part[1][2]) + s_part[1][3]) / (float)width + eps" in wg
    butterfly = int(math.log2(64))
    assert 8 * 4 + butterfly == 38 <= L_ADDS and 2 * 4 + butterfly + 3 == 17 <= L_ADDS


def test_unit_roundoffs_and_sentinels():
    v = np.random.default_rng(1).uniform(1, 2, 100000).astype(np.float32)
    assert 2.0 ** -9 < (np.abs(bf16_round(v).astype(np.float64) - v) / v).max() <= U16
    assert 2.0 ** -12 < (np.abs(f16_round(v).astype(np.float64) - v) / v).max() <= UH
    assert SENT_BF16 < 0 and abs(SENT_BF16) < 1e-15 and abs(SENT_F16 + 0.02204) < 1e-5 and abs(SENT_F32) < 1e-15


RESTATED = [(w, wg, f16, delta, n) for w in WIDTHS for wg in (0, 1) for f16 in (1, 0) for delta, n in (("none", 0), ("bf16", 0), ("parts", 4))]


@pytest.mark.parametrize("width", WIDTHS)
def test_layernorm_restatement_stays_within_the_bound(width):
    """Both kernels' summation orders in numpy float32, every family, three delta forms, both x types: inside the bound."""
    top = {}
    for w, wg, f16, delta, n in RESTATED:
        if w != width:
            continue
        x, terms, gamma, beta, fams = ln_operands(width, 5, f16, delta, n, 0, seed=1)
        ref, E = ln_reference(x, terms, delta, gamma, beta)
        y, yb = restate_layernorm(ln_v32(x, terms, delta), gamma, beta, wg)
        r32, rb = ratios(y, ref, E).max(axis=1), ratios(yb, ref, bf16_bound(ref, E)).max(axis=1)
        for i, f in enumerate(fams):
            top[f] = np.maximum(top.get(f, 0), [r32[i], rb[i]])
    for f in FAMILIES:
        print("width %4d %-8s largest ratio: fp32 %.3f, bf16 %.3f" % (width, f, *top[f]))
        assert top[f][0] <= 1.0 and top[f][1] <= 1.0, (f, top[f])


# (variant, the family that must show it, width, delta form, which output)
WRONG = [("width-1", "normal", 260, "none", "f32"), ("width-1", "massive", 4, "bf16", "f32"),
         ("dropped-piece", "normal", 260, "none", "f32"), ("dropped-piece", "offset", 1152, "bf16", "f32"),
         ("f16-stats", "offset", 1152, "bf16", "f32"), ("f16-stats", "offset", 2048, "parts", "f32"),
         ("bf16-step", "normal", 1152, "none", "bf16"), ("bf16-step", "massive", 2048, "parts", "bf16")]


@pytest.mark.parametrize("variant,family,width,delta,which", WRONG)
def test_wrong_layernorm_variants_exceed_the_bound(variant, family, width, delta, which):
    shift = FAMILIES.index(family)
    x, terms, gamma, beta, fams = ln_operands(width, 1, 0 if variant == "f16-stats" else 1, delta, 2 if delta == "parts" else 0, shift, seed=2)
    assert fams == [family]
    ref, E = ln_reference(x, terms, delta, gamma, beta)
    v = ln_v32(x, terms, delta)
    pick = (lambda r: r[0]) if which == "f32" else (lambda r: r[1])
    bound = E if which == "f32" else bf16_bound(ref, E)
    good = ratios(pick(restate_layernorm(v, gamma, beta)), ref, bound).max()
    bad = ratios(pick(restate_layernorm(v, gamma, beta, variant=variant)), ref, bound).max()
    print("%s on %s, width %d: ratio %.3g (the kernel's arithmetic: %.3g)" % (variant, family, width, bad, good))
    assert good <= 1.0 < bad
    if variant != "bf16-step":
        assert bad > 3.0


def test_missing_eps_shows_only_on_the_eps_dominated_family():
    """Why that family exists: without eps the others stay inside the bound (the constant row gives NaN)."""
    for family in ("normal", "massive", "offset", "eps"):
        x, terms, gamma, beta, fams = ln_operands(1152, 1, 1, "none", 0, FAMILIES.index(family), seed=3)
        ref, E = ln_reference(x, terms, "none", gamma, beta)
        bad = ratios(restate_layernorm(x, gamma, beta, eps=0.0)[0], ref, E).max()
        print("no eps, %-8s ratio %.3g" % (family, bad))
        assert (bad > 3.0) == (family == "eps")
    x, terms, gamma, beta, fams = ln_operands(1152, 1, 1, "none", 0, FAMILIES.index("constant"), seed=3)
    assert np.isnan(restate_layernorm(x, gamma, beta, eps=0.0)[0]).all()


def test_constant_row_and_write_back_are_exact_in_the_restatement():
    x, terms, gamma, beta, fams = ln_operands(1152, 1, 1, "none", 0, FAMILIES.index("constant"))
    for wg in (0, 1):
        y, yb = restate_layernorm(x, gamma, beta, wg)
        assert_same_bits(y, beta[None, :], "constant row")
        assert_same_bits(yb, bf16_round(beta)[None, :], "constant row, bf16")
    x, terms, gamma, beta, fams = ln_operands(260, 5, 1, "parts", 4, 0)
    assert fams[4] == "constant" and (ln_v32(x, terms, "parts")[4] == 3.0).all()     # the slabs and the bias cancel exactly


def small_linear_reference(x, w, bias, family):
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64)
    ref = x64 @ w64.T + b64
    S = np.abs(x64) @ np.abs(w64).T + np.abs(b64)
    K = x.shape[1]
    return ref, (-(-K // 64) + 8) * U * S + U * np.abs(ref)


def small_linear_operands(family, B, N, K):
    rng = np.random.default_rng([B, N, K, len(family)])
    if family == "int":
        return (rng.integers(-8, 9, (B, K)).astype(np.float32), rng.integers(-8, 9, (N, K)).astype(np.float32),
                rng.integers(-16, 17, N).astype(np.float32))
    return (rng.standard_normal((B, K)).astype(np.float32), bf16_round((rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)),
            (0.3 * rng.standard_normal(N)).astype(np.float32))


def restate_small_linear(x, w, bias):
    """small_linear_kernel in float32: lane l adds k = l, l + 64, ... with fmaf (one rounding each: float64 product, float32 sum),
    the butterfly, then the bias."""
    B, K = x.shape
    N = w.shape[0]
    lanes = np.arange(64)
    s = np.zeros((B, N, 64), np.float32)
    for k0 in range(0, K, 64):
        n = min(64, K - k0)
        prod = x[:, None, k0:k0 + n].astype(np.float64) * w[None, :, k0:k0 + n].astype(np.float64)
        s[:, :, :n] = (s[:, :, :n].astype(np.float64) + prod).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ o]
    return s[:, :, 0] + bias[None, :]


def l2norm_reference(x):
    x64 = x.astype(np.float64)
    ref = x64 / np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
    W = x.shape[1]
    b32 = np.abs(ref) * (1.01 * 0.5 * (-(-W // 64) + 7) * U + 3 * U)
    return ref, b32, b32 + UH * np.abs(ref) + 2.0 ** -25


def l2norm_operands(width):
    rng = np.random.default_rng([width, 12])
    x = rng.standard_normal((3, width)).astype(np.float32)
    x *= np.array([[1e-3], [1.0], [1e3]], np.float32) / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return x


def restate_l2norm(x):
    B, W = x.shape
    lanes = np.arange(64)
    s = np.zeros((B, 64), np.float32)
    for k0 in range(0, W, 64):
        n = min(64, W - k0)
        v = x[:, k0:k0 + n].astype(np.float64)
        s[:, :n] = (s[:, :n].astype(np.float64) + v * v).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    inv = (np.float32(1.0) / np.sqrt(s[:, :1])).astype(np.float32)
    return x * inv


@pytest.mark.parametrize("K", LINEAR_KS)
def test_small_linear_and_l2norm_bounds_are_sound_and_not_vacuous(K):
    """The kernels' arithmetic in float32 stays inside; a result one part in 2^18 off (small_linear: of S) does not."""
    x, w, bias = small_linear_operands("gauss", 3, 5, K)
    ref, bound = small_linear_reference(x, w, bias, "gauss")
    y = restate_small_linear(x, w, bias)
    S = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias)
    assert ratios(y, ref, bound).max() <= 1.0 < ratios(y + 2.0 ** -18 * S, ref, bound).max()
    xi, wi, bi = small_linear_operands("int", 3, 5, K)
    assert_same_bits(restate_small_linear(xi, wi, bi), (xi.astype(np.float64) @ wi.astype(np.float64).T + bi).astype(np.float32), "integers")
    x = l2norm_operands(K)
    ref, b32, b16 = l2norm_reference(x)
    y = restate_l2norm(x)
    assert ratios(y, ref, b32).max() <= 1.0 < ratios(y * np.float32(1 + 2.0 ** -18), ref, b32).max()
    y16 = f16_round(y)
    big = np.abs(ref) > 2.0 ** -14
    assert ratios(y16, ref, b16).max() <= 1.0
    if big.any():
        assert ratios((y16.astype(np.float16).view(np.uint16) + np.uint16(1)).view(np.float16).astype(np.float32), ref, b16)[big].max() > 1.0


def test_hooks_refuse_what_the_launchers_refuse(mse):
    """Refused before anything is allocated: this runs without a GPU."""
    from mse import ffi
    L = ffi.lib()
    buf = np.zeros(1 << 16, np.float32)
    f = _p(buf)
    assert L.mse_debug_siglip_layernorm(None) == -1 and "null argument" in ffi.last_error()

    def ln(**kw):
        a = ffi.DebugSiglipLayernormArgs()
        a.rows, a.width, a.ldx, a.x_is_f16, a.ldo, a.wg, a.eps = 2, 8, 8, 1, 8, 0, EPS
        a.x = a.gamma = a.beta = a.x_out = a.out = f
        for k, v in kw.items():
            setattr(a, k, v)
        return L.mse_debug_siglip_layernorm(C.byref(a)), ffi.last_error()

    for change, text in ((dict(width=6), "width must be a multiple of 4"), (dict(width=2052, ldx=2052, ldo=2052), "at most 2048"),
                         (dict(parts=f, bias=f, n_parts=2, part_rows=2, ldp=8, delta=f, ldd=8), "parts exclude a bf16 delta"),
                         (dict(parts=f, bias=f, n_parts=0, part_rows=2, ldp=8), "n_parts >= 1"),
                         (dict(parts=f, n_parts=2, part_rows=2, ldp=8), "a bias"),
                         (dict(parts=f, bias=f, n_parts=2, part_rows=2, ldp=10), "ldp % 4"),
                         (dict(rows=0), "rows"), (dict(ldx=4), "ldx"), (dict(ldo=10), "ldo"), (dict(wg=2), "wg"), (dict(eps=0.0), "eps"),
                         (dict(delta=f, ldd=4), "ldd"), (dict(parts=f, bias=f, n_parts=2, part_rows=1, ldp=8), "part_rows"),
                         (dict(rows=1 << 20, ldx=1 << 10), "2^26"), (dict(out=None), "null argument"), (dict(x=None), "null argument")):
        rc, err = ln(**change)
        assert rc == -1 and "debug siglip layernorm" in err and text in err, (change, err)

    pat = lambda H=28, W=42, P=14, C3=3, k_pad=640, ts=8, img=f, out=f: (L.mse_debug_siglip_patchify(img, 1, 2, C3, H, W, P, k_pad, ts, out), ffi.last_error())
    for kw in (dict(H=13), dict(W=13), dict(k_pad=584), dict(P=0), dict(ts=0), dict(img=None), dict(H=14 << 10, W=14 << 10)):
        rc, err = pat(**kw)
        assert rc == -1 and "debug siglip patchify" in err, (kw, err)
    assert "launch_patchify" in pat(H=13)[1] and "launch_patchify" in pat(W=13)[1] and "launch_patchify" in pat(k_pad=584)[1]

    tok = np.zeros(9, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    for D in (6, 517, 1150):
        assert L.mse_debug_siglip_embed_tokens(tok, f, f, 7, 3, D, 9, f) == -1 and "launch_embed_tokens" in ffi.last_error()
    assert L.mse_debug_siglip_embed_tokens(None, f, f, 7, 3, 8, 9, f) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_embed_tokens(tok, f, f, 0, 3, 8, 9, f) == -1 and "debug siglip embed tokens" in ffi.last_error()

    for dh, dv in ((64, 80), (80, 80), (72, 96)):
        assert L.mse_debug_siglip_vt_ones_row(3, dh, dv, 32, f) == -1 and "launch_vt_ones_row" in ffi.last_error()
    assert L.mse_debug_siglip_vt_ones_row(3, 72, 80, 32, None) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_vt_ones_row(0, 72, 80, 32, f) == -1

    u8 = _pu8(np.zeros(4096, np.uint8))
    assert L.mse_debug_siglip_rgb8(u8, 0, 3, 5, 7, f) == -1 and "debug siglip rgb8" in ffi.last_error()
    assert L.mse_debug_siglip_rgb8(None, 2, 3, 5, 7, f) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_bmp24(u8, 120, 20, u8, 2, 5, 7, f) == -1 and "row_stride >= 3 W" in ffi.last_error()
    assert L.mse_debug_siglip_bmp24(u8, 100, 24, u8, 2, 5, 7, f) == -1 and "img_stride" in ffi.last_error()
    assert L.mse_debug_siglip_bmp24(u8, 120, 24, None, 2, 5, 7, f) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_f32_to_bf16_pad(f, 3, 5, 4, 256, 8, f) == -1 and "ld_in >= cols" in ffi.last_error()
    assert L.mse_debug_siglip_f32_to_bf16_pad(f, 3, 5, 7, 2, 8, f) == -1 and L.mse_debug_siglip_f32_to_bf16_pad(f, 3, 5, 7, 256, 4, f) == -1
    assert L.mse_debug_siglip_f32_to_bf16_pad(f, 3, 5, 7, 1 << 14, 1 << 14, f) == -1 and "2^26" in ffi.last_error()
    assert L.mse_debug_siglip_small_linear(f, 4, f, 8, f, 8, 5, 3, 5, f) == -1 and "debug siglip small linear" in ffi.last_error()
    assert L.mse_debug_siglip_small_linear(f, 8, f, 8, f, 8, 5, 3, 4, f) == -1 and L.mse_debug_siglip_small_linear(f, 8, f, 8, None, 8, 5, 3, 5, f) == -1
    assert L.mse_debug_siglip_l2norm(f, 4, 8, 3, 1, f, f) == -1 and "debug siglip l2norm" in ffi.last_error()
    assert L.mse_debug_siglip_l2norm(f, 8, 8, 3, 2, f, f) == -1 and L.mse_debug_siglip_l2norm(f, 8, 8, 3, 1, None, None) == -1


def test_hook_comment_states_what_a_launch_writes():
    """The GPU tests below hold the kernels to this text; it must not drift from them silently."""
    src = " ".join(_source("siglip_api.hip").replace("//", " ").split())
    for sentence in (
            "each call makes ONE call of the launcher the towers use",
            "the columns between the width and the leading dimension of an OPERAND hold 1e4",
            "with NO delta x is not written at all",
            "Columns width .. ld keep the sentinel",
            "columns >= C P P and rows t >= tokens of an image are ZEROED",
            "pixels past the last whole patch are ignored",
            "rows >= rows and columns >= cols are ZEROED",
            "columns N .. ldy keep the sentinel",
            "EVERYTHING else keeps the sentinel",
            "is refused before anything is allocated"):
        assert sentence in src, sentence


# ---------------------------------------------------------------------------------------------------------
# GPU: LayerNorm
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted({(c[0], c[3], c[2]) for c in LN_GRID}) + [("tower", 0, 1)], ids=lambda k: "w%s-wg%d-%s" % (k[0], k[1], "f16" if k[2] else "f32"))
def test_layernorm_against_float64(gpu, key):
    cases = LN_TOWER if key[0] == "tower" else [c for c in LN_GRID if (c[0], c[3], c[2]) == key]
    top = {}
    for case in cases:
        width, rows, x_is_f16, wg, delta, n_parts, outs, ldx, ldd, ldp, ldo, shift = case
        what = ln_id(case) + " [" + kernel_of("layernorm", x_is_f16, wg) + "]"
        x, terms, gamma, beta, fams = ln_operands(width, rows, x_is_f16, delta, n_parts, shift)
        got = run_layernorm(case, x, terms, gamma, beta)
        # x: the storage-type rounding of the fp32 sum in the source's order (unchanged without a delta); the padding keeps the sentinel
        v32 = ln_v32(x, terms, delta)
        assert_same_bits(got["x"][:, :width], f16_round(v32) if x_is_f16 else v32, what + ": x written back")
        assert (got["x"][:, width:] == (SENT_F16 if x_is_f16 else SENT_F32)).all(), what + ": x columns width .. ldx were written"
        ref, E = ln_reference(x, terms, delta, gamma, beta)
        for name, bound, sent in (("out_f32", E, SENT_F32), ("out", bf16_bound(ref, E), SENT_BF16)):
            if name not in got:
                continue
            o = got[name]
            assert np.isfinite(o).all() and (o[:, width:] == sent).all(), what + ": %s columns width .. ldo were written" % name
            ratio = ratios(o[:, :width], ref, bound)
            for i, f in enumerate(fams):
                k = (name, f)
                top[k] = max(top.get(k, 0.0), float(ratio[i].max()))
            r, where = worst(o[:, :width], ref, bound)
            assert r <= 1.0, "%s %s (row families %s): %s" % (what, name, fams, where)
            for i, f in enumerate(fams):
                if f == "constant" and delta == "none":       # all its sums are exact
                    assert_same_bits(o[i, :width], beta if name == "out_f32" else bf16_round(beta), what + ": constant row, " + name)
        if "out" in got and "out_f32" in got:
            assert_same_bits(got["out"][:, :width], bf16_round(got["out_f32"][:, :width]), what + ": the bf16 output is not the rounded fp32 one")
    for (name, f) in sorted(top):
        print("layernorm w%s-wg%d-%s %-7s %-8s largest |got - ref| / bound %.3f" % (key[0], key[1], "f16" if key[2] else "f32", name, f, top[(name, f)]))


# ---------------------------------------------------------------------------------------------------------
# GPU: the exact kernels
# ---------------------------------------------------------------------------------------------------------
def decode_exact(u8_nchw):
    return (u8_nchw.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float16).astype(np.float32)


def run_rgb8(pix):
    from mse import ffi
    B, H, W, Cc = pix.shape
    out = np.full((B, Cc, H, W), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_rgb8(_pu8(np.ascontiguousarray(pix)), B, Cc, H, W, _p(out)), "mse_debug_siglip_rgb8")
    return out


@pytest.mark.gpu
def test_rgb8_decode_is_exact(gpu):
    B, H, W = 2, 5, 7
    seen = np.zeros((3, 256), bool)
    for launch in range(4):        # 70 pixels a launch: four launches walk all 256 byte values through every channel
        n = np.arange(B * H * W).reshape(B, H, W, 1)
        pix = ((n + 70 * launch + 85 * np.arange(3)) % 256).astype(np.uint8)
        for c in range(3):
            seen[c, pix[..., c].ravel()] = True
        assert_same_bits(run_rgb8(pix), decode_exact(pix.transpose(0, 3, 1, 2)), "rgb8 launch %d" % launch)
    assert seen.all(), "byte values never decoded: %s" % np.argwhere(~seen)[:8].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [7, 8])
def test_bmp24_decode_is_exact(gpu, W):
    from mse import ffi
    B, H = 2, 5
    rng = np.random.default_rng(W)
    pix = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)          # RGB, top row first
    stride = (3 * W + 3) // 4 * 4
    assert stride == 24 and (stride - 3 * W) == (3 if W == 7 else 0)
    flags = np.array([1, 0], np.uint8)                                 # image 0 bottom-up, image 1 top-down
    raw = np.full((B, H, stride), 0xEE, np.uint8)
    for b in range(B):
        rows = pix[b, ::-1] if flags[b] else pix[b]
        raw[b, :, :3 * W] = rows[..., ::-1].reshape(H, 3 * W)          # blue, green, red
    out = np.full((B, 3, H, W), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_bmp24(_pu8(raw), H * stride, stride, _pu8(flags), B, H, W, _p(out)), "mse_debug_siglip_bmp24")
    assert_same_bits(out, decode_exact(pix.transpose(0, 3, 1, 2)), "bmp24 W %d" % W)
    assert_same_bits(out, run_rgb8(pix), "bmp24 against rgb8 of the same pixels")


def patchify_image(is_f16, shape):
    """Values whose rounding to bf16 can go wrong: ties in both directions, negatives, fp16 subnormals, carries into the exponent."""
    rng = np.random.default_rng([is_f16, *shape])
    n = int(np.prod(shape))
    if is_f16:
        h = rng.integers(0x2000, 0x4800, n).astype(np.uint16)          # 2^-7 .. 8
        h[0::5] = (h[0::5] & np.uint16(0xFFF8)) | np.uint16(0x4)        # low three bits 100: a tie, up or down by bit 3
        h[2::11] |= np.uint16(0x03FC)                                   # mantissa ones down to the tie bit: the carry reaches the exponent
        h[1::7] &= np.uint16(0x03FF)                                    # subnormals
        h |= (rng.integers(0, 2, n) << 15).astype(np.uint16)
        img = h.view(np.float16).astype(np.float32)
        assert (np.abs(img[1::7]) < 2.0 ** -14).all()
    else:
        img = rng.standard_normal(n).astype(np.float32)
        u = img.view(np.uint32)
        u[0::5] = (u[0::5] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)     # exact ties
        u[2::11] = (u[2::11] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
        u[1::7] = (u[1::7] & np.uint32(0xFF800000)) | np.uint32(0x7FFFFF)   # just below a power of two: rounds up to it
        assert (np.abs(bf16_round(img[1::7])) == 2.0 ** np.round(np.log2(np.abs(bf16_round(img[1::7]))))).all()
    assert (img < 0).any() and np.isfinite(img).all()
    return img.reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PATCHIFY_CASES, ids=lambda c: "P%d-C%d-%dx%d-k%d" % c[:5])
@pytest.mark.parametrize("is_f16", [1, 0], ids=["f16", "f32"])
def test_patchify_is_exact(gpu, case, is_f16):
    from mse import ffi
    P, Cc, H, W, k_pad, B, ts = case
    gh, gw = H // P, W // P
    img = patchify_image(is_f16, (B, Cc, H, W))
    want = np.zeros((B, ts, k_pad), np.float32)
    want[:, :gh * gw, :Cc * P * P] = bf16_round(img)[:, :, :gh * P, :gw * P].reshape(B, Cc, gh, P, gw, P).transpose(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, Cc * P * P)
    out = np.full((B, ts, k_pad), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_patchify(_p(img), is_f16, B, Cc, H, W, P, k_pad, ts, _p(out)), "mse_debug_siglip_patchify")
    assert (out != SENT_BF16).all(), "patchify left %d elements unwritten" % (out == SENT_BF16).sum()
    assert_same_bits(out, want, "patchify [%s]" % kernel_of("patchify", P, k_pad, is_f16))


@pytest.mark.gpu
@pytest.mark.parametrize("D", EMBED_WIDTHS)
def test_embed_tokens_is_exact(gpu, D):
    from mse import ffi
    vocab, ctx, B = 7, 3, 3
    rng = np.random.default_rng(D)
    emb = rng.standard_normal((vocab, D)).astype(np.float32)
    pos = rng.standard_normal((ctx, D)).astype(np.float32)
    tokens = np.array([3, -1, 6, vocab, 1, 2 ** 40, 0, 5, 2], np.int64)
    out = np.full((B * ctx, D), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_embed_tokens(tokens.ctypes.data_as(C.POINTER(C.c_int64)), _p(emb), _p(pos), vocab, ctx, D, B * ctx, _p(out)),
              "mse_debug_siglip_embed_tokens")
    tk = np.where((tokens < 0) | (tokens >= vocab), 0, tokens)            # out-of-range tokens read row 0 (the kernel's stated behaviour)
    assert_same_bits(out, f16_round(emb[tk] + pos[np.arange(B * ctx) % ctx]), "embed_tokens D %d" % D)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: "%dx%d-ld%d-to-%dx%d" % c)
def test_f32_to_bf16_pad_is_exact(gpu, case):
    from mse import ffi
    rows, cols, ld_in, rows_pad, cols_pad = case
    rng = np.random.default_rng(rows)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    u = x.view(np.uint32)
    u[:, 0] = (u[:, 0] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    u[:, -1] = (u[:, -1] & np.uint32(0xFFFE0000)) | np.uint32(0x18000)
    out = np.full((rows_pad, cols_pad), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_f32_to_bf16_pad(_p(x), rows, cols, ld_in, rows_pad, cols_pad, _p(out)), "mse_debug_siglip_f32_to_bf16_pad")
    want = np.zeros((rows_pad, cols_pad), np.float32)
    want[:rows, :cols] = bf16_round(x)
    assert_same_bits(out, want, "f32_to_bf16_pad")


@pytest.mark.gpu
@pytest.mark.parametrize("n_pad", VT_PADS)
def test_vt_ones_row_writes_row_72_only(gpu, n_pad):
    from mse import ffi
    out = np.full((3, 80, n_pad), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_vt_ones_row(3, 72, 80, n_pad, _p(out)), "mse_debug_siglip_vt_ones_row")
    want = np.full((3, 80, n_pad), SENT_BF16, np.float32)
    want[:, 72, :] = 1.0
    assert_same_bits(out, want, "vt_ones_row n_pad %d" % n_pad)


# ---------------------------------------------------------------------------------------------------------
# GPU: small_linear and l2norm
# ---------------------------------------------------------------------------------------------------------
def run_small_linear(x, w, bias, ldx, ldw, ldy):
    from mse import ffi
    B, K = x.shape
    N = w.shape[0]
    y = np.full((B, ldy), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_small_linear(_p(np.ascontiguousarray(x)), ldx, _p(np.ascontiguousarray(w)), ldw, _p(bias), K, N, B, ldy, _p(y)),
              "mse_debug_siglip_small_linear")
    assert (y[:, N:] == SENT_F32).all(), "small_linear wrote columns N .. ldy"
    return y[:, :N]


@pytest.mark.gpu
@pytest.mark.parametrize("K", LINEAR_KS)
@pytest.mark.parametrize("B,N", LINEAR_SHAPES)
def test_small_linear_against_float64(gpu, B, N, K):
    for ldx, ldw, ldy in ((K, K, N), (K + 3, K + 5, N + 2)):
        x, w, bias = small_linear_operands("int", B, N, K)
        exact = (x.astype(np.float64) @ w.astype(np.float64).T + bias).astype(np.float32)
        assert_same_bits(run_small_linear(x, w, bias, ldx, ldw, ldy), exact, "small_linear, integers: must be the exact value")
        x, w, bias = small_linear_operands("gauss", B, N, K)
        ref, bound = small_linear_reference(x, w, bias, "gauss")
        r, where = worst(run_small_linear(x, w, bias, ldx, ldw, ldy), ref, bound)
        print("small_linear B %d N %d K %d ld +%d gauss largest |got - ref| / bound %.3f" % (B, N, K, ldx - K, r))
        assert r <= 1.0, where


@pytest.mark.gpu
def test_small_linear_hook_rounds_w_as_numpy_does(gpu):
    """x = unit vectors read rows of w back: the hook's bf16 rounding, ties and odd mantissas included."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((5, 70)).astype(np.float32)
    u = w.view(np.uint32)
    u[0] = (u[0] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    u[1] = (u[1] & np.uint32(0xFFFE0000)) | np.uint32(0x18000)
    u[2] = (u[2] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
    cols = (0, 63, 69)
    x = np.zeros((3, 70), np.float32)
    x[np.arange(3), cols] = 1.0
    got = run_small_linear(x, w, np.zeros(5, np.float32), 72, 71, 5)
    assert_same_bits(got, bf16_round(w)[:, cols].T, "w rounding")


def run_l2norm(x, ldx, normalize, want32=True, want16=True):
    from mse import ffi
    B, W = x.shape
    o32 = np.full((B, W), np.nan, np.float32) if want32 else None
    o16 = np.full((B, W), np.nan, np.float32) if want16 else None
    ffi.check(ffi.lib().mse_debug_siglip_l2norm(_p(np.ascontiguousarray(x)), ldx, W, B, normalize, _p(o32) if want32 else None,
                                                _p(o16) if want16 else None), "mse_debug_siglip_l2norm")
    return o32, o16


@pytest.mark.gpu
@pytest.mark.parametrize("W", L2_WIDTHS)
def test_l2norm_against_float64(gpu, W):
    x = l2norm_operands(W)
    ref, b32, b16 = l2norm_reference(x)
    for ldx in (W, W + 3):
        o32, o16 = run_l2norm(x, ldx, 1)
        r32, where32 = worst(o32, ref, b32)
        r16, where16 = worst(o16, ref, b16)
        print("l2norm W %d ld +%d largest |got - ref| / bound: fp32 %.3f, fp16 %.3f" % (W, ldx - W, r32, r16))
        assert r32 <= 1.0, where32
        assert r16 <= 1.0, where16
        assert_same_bits(o16, f16_round(o32), "l2norm: the fp16 output is not the rounded fp32 one")
    only32, none16 = run_l2norm(x, W + 3, 1, want16=False)
    none32, only16 = run_l2norm(x, W + 3, 1, want32=False)
    assert none16 is None and none32 is None
    assert_same_bits(only32, o32, "l2norm, fp32 output alone")
    assert_same_bits(only16, o16, "l2norm, fp16 output alone")


@pytest.mark.gpu
def test_l2norm_exact_cases(gpu):
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((3, 70)) * np.array([[1e-3], [1.0], [1e3]])).astype(np.float32)
    o32, o16 = run_l2norm(x, 75, 0)
    assert_same_bits(o32, x, "normalize = 0: fp32 output")
    assert_same_bits(o16, f16_round(x), "normalize = 0: fp16 output")
    e = np.zeros((3, 70), np.float32)
    e[np.arange(3), (0, 64, 69)] = (1.0, -1.0, 1.0)
    o32, o16 = run_l2norm(e, 70, 1)
    assert_same_bits(o32, e, "a unit basis vector")
    assert_same_bits(o16, e, "a unit basis vector, fp16")
