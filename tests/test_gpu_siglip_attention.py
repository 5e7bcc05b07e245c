"""SigLIP attention where trained weights put the softmax: the self-attention kernel (attention64_kernel, its three shipped tilings) and the
pooling attention against a float64 softmax attention over the same bf16-rounded operands, with a DERIVED tolerance, on logits that reach
the data-dependent half of the kernel -- the lazy, wave-voted running maximum -- and one end-to-end check per tower with the
q projections sharpened.

Kernel tests go through mse_debug_siglip_attention / mse_debug_siglip_pool_attention (the launchers the towers call, the QKV epilogue's
layouts).  Per output element, with w the float64 softmax weights of the row, A[e] = sum_t w_t |v_t[e]| and
L1 = max_t sum_i |q_i k_ti| / sqrt(72):

    self attention   |got - ref| <= 2 * (2 eps / (1 - eps)) * A[e] + 2^-7 |ref[e]| + 1e-30,    eps = 2^-8 + 80 * 2^-24 * L1
    pooling          |got - ref| <= 4 * 2 eps * A[e] + 2^-20 |ref[e]|,                         eps = 80 * 2^-24 * L1 + 2^-20

2^-8: p rounded (or truncated) to bf16, numerator and row sum alike; 80 * 2^-24 * L1: fp32 accumulation of a logit of 72 exact products;
2^-7 |ref|: the bf16 store, same allowance; the leading 2 (4 for the pooling kernel's longer fp32 sums) is the only margin and covers
exp2 / rcp.  Every family keeps eps <= 2^-7 (asserted), so no family loosens its own tolerance.

Families (logits in log2 units, l2 = q.k / sqrt(72) * log2(e); structure in the first four of the 72 dimensions, Gaussian noise in the
other 68): gauss (N(0, 1), the regime of the seeded weights: no rescale after the first 32 keys), stairs_up (the row maximum rises by
12 every 32 keys: a rescale at every half), stairs_down (maximum in the first 32 keys, the rest 110 lower), spike (one key 60 above the
rest; a different position per head: 0, 31, 32, 63, 64, tokens - 1, first key of the last half), spike_some (only query rows i with
i % 16, i % 5 or i % 37 == 0 have a spike: one lane votes, the whole wave rescales), threshold (a rise of 7.9 / 8.1 at the second half,
alternating by 32-row groups), offset_pos / offset_neg (all logits within 2 of +200 / -200), gauss8 / gauss16 (N(0, 1) scaled).

Largest |got - ref| / bound measured on an MI355X, per family (self attention, over all its shapes; the bound is 1):
    gauss 0.155, stairs_up 0.214, stairs_down 0.158, spike 0.000, spike_some 0.227, threshold 0.170, offset_pos 0.091, offset_neg 0.150,
    gauss8 0.275, gauss16 0.276 (the largest: 3 images of 729 tokens, the <2, 8> tiling)
pooling attention:
    gauss 0.001, spike 0.000, offset_neg 0.003, gauss16 0.005
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

torch.set_grad_enabled(False)

DH = 72
LOG2E = 1.4426950408889634
UNIT = math.sqrt(DH) / LOG2E          # the q.k that is one log2 unit of logit
N_STRUCT = 4                          # leading dimensions that carry a family's structure; the rest carry noise
HALF = 32                             # keys per softmax step of attention64_kernel
VOTE = 8.0                            # a lane votes when its score is more than 2^8 above the running maximum


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def round_up(v, m):
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------
# the float64 reference (with what the tolerance and the regime conditions need)
# ---------------------------------------------------------------------------------------------------------
def vote_events(l2):
    """The lazy maximum of ONE query row, 32-key halves in key order: after the first half the running maximum is raised only when a
    half's maximum is more than VOTE above it.  l2: [..., tokens] logits in log2 units; returns the number of raises per row."""
    t = l2.shape[-1]
    n_half = (t + HALF - 1) // HALF
    pad = np.full(l2.shape[:-1] + (n_half * HALF,), -np.inf)
    pad[..., :t] = l2
    hm = pad.reshape(l2.shape[:-1] + (n_half, HALF)).max(-1)
    m, ev = hm[..., 0].copy(), np.zeros(l2.shape[:-1], np.int64)
    for j in range(1, n_half):
        rise = hm[..., j] - m > VOTE
        ev += rise
        m = np.where(rise, np.maximum(m, hm[..., j]), m)
    return ev


class Ref:
    """out, A: [B][tokens_q][heads * 72]; L1, events, wmax (largest weight of a row), tail (weight past the first 32 keys):
    [B][heads][tokens_q]; l2_min / l2_max over everything."""


def reference(q, k, v):
    """q [B][heads][nq][72], k / v [B][heads][tokens][72]: the values the kernel multiplies (already rounded), any float dtype."""
    B, H, nq, _ = q.shape
    r = Ref()
    r.out, r.A = np.empty((B, nq, H * DH)), np.empty((B, nq, H * DH))
    r.L1, r.wmax, r.tail = np.empty((B, H, nq)), np.empty((B, H, nq)), np.empty((B, H, nq))
    r.events = np.empty((B, H, nq), np.int64)
    r.l2_min, r.l2_max = np.inf, -np.inf
    for b in range(B):
        qd, kd, vd = (np.asarray(x[b], np.float64) for x in (q, k, v))
        kt = kd.transpose(0, 2, 1)
        s = qd @ kt / math.sqrt(DH)
        r.L1[b] = (np.abs(qd) @ np.abs(kt)).max(-1) / math.sqrt(DH)
        r.l2_min, r.l2_max = min(r.l2_min, s.min() * LOG2E), max(r.l2_max, s.max() * LOG2E)
        r.events[b] = vote_events(s * LOG2E)
        s -= s.max(-1, keepdims=True)
        np.exp(s, out=s)
        s /= s.sum(-1, keepdims=True)
        r.wmax[b], r.tail[b] = s.max(-1), s[..., HALF:].sum(-1)
        o = s @ np.concatenate([vd, np.abs(vd)], axis=-1)                    # [H][nq][144]
        r.out[b] = o[..., :DH].transpose(1, 0, 2).reshape(nq, H * DH)
        r.A[b] = o[..., DH:].transpose(1, 0, 2).reshape(nq, H * DH)
    return r


def per_element(x):
    """[B][heads][nq] -> [B][nq][heads * 72]"""
    return np.repeat(x.transpose(0, 2, 1), DH, axis=-1)


def self_bound(r):
    eps = per_element(2.0 ** -8 + 80 * 2.0 ** -24 * r.L1)
    return 2 * (2 * eps / (1 - eps)) * r.A + 2.0 ** -7 * np.abs(r.out) + 1e-30


def pool_bound(r):
    eps = per_element(80 * 2.0 ** -24 * r.L1 + 2.0 ** -20)
    return 4 * 2 * eps * r.A + 2.0 ** -20 * np.abs(r.out)


# ---------------------------------------------------------------------------------------------------------
# the key families
# ---------------------------------------------------------------------------------------------------------
NOISE = {"gauss": 1.0, "stairs_up": 1.0, "stairs_down": 1.0, "spike": 1.0, "spike_some": 1.0, "threshold": 0.01,
         "offset_pos": 0.3, "offset_neg": 0.3, "gauss8": 8.0, "gauss16": 16.0}
FAMILIES = list(NOISE)
SPIKE = 60.0
SOME = (16, 5, 37)                    # spike_some: query rows i with i % m == 0 carry the spike of class m


@functools.lru_cache(maxsize=None)
def _noise(B, H, T):
    g = np.random.Generator(np.random.Philox(key=0x5EED0A11 + 1000003 * B + 1009 * H + T))
    out = tuple(g.standard_normal((B, H, T, DH), dtype=np.float32) for _ in range(3))
    for a in out:
        a.flags.writeable = False
    return out


def spike_positions(T):
    want = [0, 31, 32, 63, 64, T - 1, (T - 1) // HALF * HALF]
    return sorted({p for p in want if 0 <= p < T})


def some_positions(bh, T):
    """the key of the spike of each class of spike_some, per (image, head)"""
    return [(7 * bh + 3) % T, (13 * bh + 40) % T, (29 * bh + T // 2) % T]


def threshold_rise(i):
    return 7.9 if (i // 32) % 2 == 0 else 8.1


def build(family, B, H, T, pool=False):
    """q, k, v float32 [B][heads][tokens][72], NOT yet rounded to bf16 (the hook rounds; the reference rounds in numpy).  pool: one
    query per head, the same for every image (q [B][heads][1][72])."""
    gq, gk, gv = _noise(B, H, T)
    sig = math.sqrt(NOISE[family] * UNIT / math.sqrt(DH - N_STRUCT))         # noise logits ~ N(0, NOISE^2) log2 units
    k = np.zeros((B, H, T, DH), np.float32)
    k[..., N_STRUCT:] = gk[..., N_STRUCT:] * sig
    nq = 1 if pool else T
    q = np.zeros((B, H, nq, DH), np.float32)
    q[..., N_STRUCT:] = (gq[:1, :, :1] if pool else gq)[..., N_STRUCT:] * sig
    v = gv.copy()
    t = np.arange(T)
    if family in ("stairs_up", "stairs_down"):
        target = 12.0 * (t // HALF) - 6.0 * ((T - 1) // HALF) if family == "stairs_up" else np.where(t < HALF, 0.0, -110.0)
        q[..., 0] = 8.0
        k[..., 0] = target * UNIT / 8.0
    elif family in ("offset_pos", "offset_neg"):
        q[..., 0] = 200.0 * UNIT / 16.0
        k[..., 0] = 16.0 if family == "offset_pos" else -16.0
    elif family == "spike":
        pos = spike_positions(T)
        q[..., 1] = 8.0
        for bh in range(B * H):
            k[bh // H, bh % H, pos[bh % len(pos)], 1] = SPIKE * UNIT / 8.0
    elif family == "spike_some":
        for c, m in enumerate(SOME):
            q[:, :, ::m, 1 + c] = 8.0
            for bh in range(B * H):
                k[bh // H, bh % H, some_positions(bh, T)[c], 1 + c] = SPIKE * UNIT / 8.0
    elif family == "threshold":
        q[..., 1] = np.array([threshold_rise(i) for i in range(nq)], np.float32) * UNIT
        for bh in range(B * H):
            k[bh // H, bh % H, HALF + bh % min(HALF, T - HALF), 1] = 1.0
    return q, k, v


def check_regime(family, T, r, nq_rows=None):
    """What a family must be on the REFERENCE (conditions, not measurements), and the cap that keeps its tolerance from loosening."""
    eps = 2.0 ** -8 + 80 * 2.0 ** -24 * r.L1.max()
    assert eps <= 2.0 ** -7, (family, eps)
    n_half = round_up(T, HALF) // HALF
    ev = r.events
    if family == "gauss":
        assert ev.max() == 0
    elif family == "stairs_up":
        assert ev.min() >= n_half - 2, (ev.min(), n_half)
    elif family == "stairs_down":
        assert ev.max() == 0 and r.tail.max() <= T * 2.0 ** -100, r.tail.max()
    elif family == "spike":
        assert r.wmax.min() >= 1 - T * 2.0 ** -40, r.wmax.min()
    elif family == "spike_some" and nq_rows is None:
        rows = np.arange(ev.shape[-1])
        some = np.zeros(ev.shape[-1], bool)
        for m in SOME:
            some |= rows % m == 0
        assert ev[..., ~some].max() == 0
        if T > HALF:
            assert (ev[..., some] > 0).mean() >= 0.25, (ev[..., some] > 0).mean()
    elif family == "threshold" and nq_rows is None:
        low = np.array([threshold_rise(i) < VOTE for i in range(ev.shape[-1])])
        assert ev[..., low].max() == 0 and ev[..., ~low].min() == 1 and ev[..., ~low].max() == 1
    elif family in ("offset_pos", "offset_neg"):
        c = 200.0 if family == "offset_pos" else -200.0
        assert c - 2 <= r.l2_min and r.l2_max <= c + 2, (r.l2_min, r.l2_max)
        if family == "offset_neg":
            assert r.wmax.max() < 0.2, r.wmax.max()        # a leaked zero-logit padding key would own the row
    elif family == "gauss8" and T == 729:
        assert (ev > 0).mean() >= 0.5, (ev > 0).mean()


@functools.lru_cache(maxsize=3)
def case(family, B, H, T):
    """(q, k, v) as given to the hook and the float64 reference over their bf16 roundings; built once, shared, read-only."""
    q, k, v = build(family, B, H, T)
    r = reference(bf16_round(q), bf16_round(k), bf16_round(v))
    for a in (q, k, v, r.out, r.A, r.L1, r.events, r.wmax, r.tail):
        a.flags.writeable = False
    return q, k, v, r


# smallest shapes that reach each tiling and boundary (launch_attention chooses by B * heads and tokens); n_pad = tokens rounded to 32
SHAPES_QT1_NW4 = [(1, 16, t) for t in (17, 32, 33, 64, 65, 97, 729)]
SHAPES_QT1_NW8 = [(4, 16, 200), (2, 16, 729)]
SHAPES_QT2_NW8 = [(8, 16, 96), (8, 16, 257), (3, 16, 729)]
SHAPE_NO_REMAP = [(1, 3, 96)]         # heads % 8 != 0: the branch without the XCD remap
ALL_FAMILIES_AT = [(1, 16, 64), (1, 16, 729), (8, 16, 96), (3, 16, 729)]
SOME_FAMILIES = ["gauss", "stairs_up", "spike", "offset_neg"]
SELF_CASES = [(f, *s) for s in SHAPES_QT1_NW4 + SHAPES_QT1_NW8 + SHAPES_QT2_NW8 + SHAPE_NO_REMAP
              for f in (FAMILIES if s in ALL_FAMILIES_AT else SOME_FAMILIES)]


def tiling(B, H, T):
    """launch_attention's choice restated: (query tiles per wave, waves per workgroup)"""
    if B * H * ((T + 255) // 256) < 128 or T <= 64:
        return (1, 4) if T <= 64 or B * H * ((T + 127) // 128) < 128 else (1, 8)
    return (2, 8)


def test_the_shapes_reach_the_three_tilings():
    assert {tiling(*s) for s in SHAPES_QT1_NW4 + SHAPE_NO_REMAP} == {(1, 4)}
    assert {tiling(*s) for s in SHAPES_QT1_NW8} == {(1, 8)} and {tiling(*s) for s in SHAPES_QT2_NW8} == {(2, 8)}
    assert {tiling(*s) for s in ALL_FAMILIES_AT} == {(1, 4), (2, 8)}
    assert len(SELF_CASES) == 4 * len(FAMILIES) + 9 * len(SOME_FAMILIES)


@pytest.mark.parametrize("family,T", [(f, 64) for f in FAMILIES] + [("gauss", 729), ("stairs_up", 729), ("gauss8", 729)])
def test_families_are_in_their_regime(family, T):
    """On the reference alone: stairs_up raises the maximum at (all but at most one of) the halves after the first in EVERY row (22 halves
    follow the first at 729 tokens), gauss never, gauss8 in at least half of the rows at 729 tokens; spikes, thresholds and offsets are
    what their names say; eps stays under its cap."""
    _, _, _, r = case(family, 1, 16, T)
    check_regime(family, T, r)
    print(family, T, "rows with a raise after the first half: %.3f, raises per row %d..%d, L1 max %.1f" %
          ((r.events > 0).mean(), r.events.min(), r.events.max(), r.L1.max()))


# ---------------------------------------------------------------------------------------------------------
# the self-attention kernel
# ---------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def run_attention(q, k, v, flags=0):
    from mse import ffi
    B, H, T, _ = q.shape
    q, k, v = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
    out = np.full((B, T, H * DH), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_attention(_p(q), _p(k), _p(v), B, H, T, flags, _p(out)), "mse_debug_siglip_attention")
    return out


def run_pool_attention(qlat, k, v):
    from mse import ffi
    B, T, D = k.shape
    qlat, k, v = (np.ascontiguousarray(x, np.float32) for x in (qlat, k, v))
    out = np.full((B, D), np.nan, np.float32)
    ffi.check(ffi.lib().mse_debug_siglip_pool_attention(_p(qlat), _p(k), _p(v), B, D // DH, T, _p(out)), "mse_debug_siglip_pool_attention")
    return out


def worst(got, r, bound):
    ratio = np.abs(got.astype(np.float64) - r.out) / bound
    i = np.unravel_index(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf)), ratio.shape)
    return float(ratio[i]), "worst at [image %d, query %d, column %d]: got %.9g, reference %.9g, bound %.3g" % (
        i[0], i[1], i[2], got[i], r.out[i], bound[i])


def test_hooks_reject_bad_arguments(mse):
    from mse import ffi
    L = ffi.lib()
    x = np.zeros(DH, np.float32)
    assert L.mse_debug_siglip_attention(None, None, None, 1, 16, 17, 0, None) == -1 and "null argument" in ffi.last_error()
    assert L.mse_debug_siglip_pool_attention(None, None, None, 1, 16, 17, None) == -1 and "null argument" in ffi.last_error()
    for B, H, T, flags in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 2), (1 << 12, 1 << 6, 1 << 5, 0)):
        assert L.mse_debug_siglip_attention(_p(x), _p(x), _p(x), B, H, T, flags, _p(x)) == -1 and "debug siglip attention" in ffi.last_error()
        if flags == 0:
            assert L.mse_debug_siglip_pool_attention(_p(x), _p(x), _p(x), B, H, T, _p(x)) == -1 and "debug siglip pool attention" in ffi.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("family,B,H,T", SELF_CASES)
def test_self_attention_against_float64(gpu, family, B, H, T):
    q, k, v, r = case(family, B, H, T)
    check_regime(family, T, r)
    got = run_attention(q, k, v)
    ratio, where = worst(got, r, self_bound(r))
    print("self attention %-11s B %d heads %2d tokens %3d tiling %s: largest |got - ref| / bound %.3f; %s" %
          (family, B, H, T, tiling(B, H, T), ratio, where))
    assert np.isfinite(got).all()
    assert ratio <= 1.0, where


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["gauss", "spike_last", "offset_neg"])
@pytest.mark.parametrize("T", [33, 97, 729])
def test_padding_content_does_not_reach_the_result(gpu, family, T):
    """Finite garbage of magnitude up to 1e4 in the padded K rows, V columns and q rows (flags = 1): the same bits as with zeros."""
    if family == "spike_last":
        q, k, v = build("gauss", 1, 16, T)
        q[..., 1] = 8.0
        k[:, :, T - 1, 1] = SPIKE * UNIT / 8.0
    else:
        q, k, v = build(family, 1, 16, T)
    clean, dirty = run_attention(q, k, v, 0), run_attention(q, k, v, 1)
    d = np.argwhere(clean != dirty)
    assert np.isfinite(clean).all()
    assert d.size == 0, "%d elements differ, the first at [image, query, column] %s: %r with zeros, %r with garbage; query rows that differ: %s" % (
        len(d), d[0].tolist(), clean[tuple(d[0])], dirty[tuple(d[0])], sorted(set(d[:, 1].tolist()))[:20])


@pytest.mark.gpu
def test_the_hook_rounds_like_numpy(gpu):
    """The reference rounds q, k and v in numpy; the hook rounds them on the host.  V directly: behind a spike of 60 the output row IS the
    rounded V row of the spike key (weight 1 - 2^-60 * tokens), so V values that sit exactly halfway between two bf16 neighbours must come
    back rounded to even.  q and K: rounding them beforehand changes no bit of the result."""
    T = 65
    q, k, v = build("gauss", 1, 16, T)
    q[..., 1] = 8.0
    k[:, :, 40, 1] = SPIKE * UNIT / 8.0
    u = v.view(np.uint32)
    u[:, :, 40, :] = (u[:, :, 40, :] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)      # exact ties, odd and even neighbours below
    got = run_attention(q, k, v)
    want = bf16_round(v[:, :, 40, :]).transpose(1, 0, 2).reshape(1, 1, 16 * DH)
    assert np.array_equal(got, np.broadcast_to(want, got.shape))
    q, k, v, _ = case("gauss8", 1, 16, 64)
    assert np.array_equal(run_attention(q, k, v), run_attention(bf16_round(q), bf16_round(k), bf16_round(v)))


# ---------------------------------------------------------------------------------------------------------
# the pooling attention (fp32 on the vector ALU)
# ---------------------------------------------------------------------------------------------------------
POOL_CASES = [(f, B, T) for B, T in ((1, 729), (3, 729), (2, 64)) for f in ("gauss", "spike", "offset_neg", "gauss16")]


def pool_spike_positions(T):
    return sorted({p for p in (0, 255, 256, T - 1) if p < T})


@pytest.mark.gpu
@pytest.mark.parametrize("family,B,T", POOL_CASES)
def test_pool_attention_against_float64(gpu, family, B, T):
    H = 16
    q, k, v = build("gauss" if family == "spike" else family, B, H, T, pool=True)
    if family == "spike":
        pos = pool_spike_positions(T)
        q[..., 1] = 8.0
        for bh in range(B * H):
            k[bh // H, bh % H, pos[bh % len(pos)], 1] = SPIKE * UNIT / 8.0
    kr, vr = bf16_round(k), bf16_round(v)
    r = reference(q, kr, vr)                      # the kernel reads the latent query in fp32
    assert (80 * 2.0 ** -24 * r.L1 + 2.0 ** -20).max() <= 2.0 ** -7
    check_regime(family, T, r, nq_rows=1)
    flat = lambda x: x.transpose(0, 2, 1, 3).reshape(B, T, H * DH)
    got = run_pool_attention(q[0, :, 0].reshape(H * DH), flat(k), flat(v))[:, None, :]
    ratio, where = worst(got, r, pool_bound(r))
    print("pool attention %-10s B %d tokens %3d: largest |got - ref| / bound %.3f; %s" % (family, B, T, ratio, where))
    assert np.isfinite(got).all()
    assert ratio <= 1.0, where


# ---------------------------------------------------------------------------------------------------------
# end to end: the towers with the q projection of every block multiplied by lambda
# ---------------------------------------------------------------------------------------------------------
DEPTH = 2
IMAGE_BATCHES = (1, 2, 5)             # the three tilings of the self attention
TEXT_BATCHES = (3, 112)
TEXT_LAMBDA = 8                       # the issue's fall-back (16 for the text tower only) is not needed: test_sharpened_text_tower_is_a_fair_input


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1)


def sharpen(sd, names, lam, d=1152):
    """a copy of the state dict with the q rows of every block's fused qkv projection (weight and bias) multiplied by lam"""
    out = dict(sd)
    for w, b in names:
        out[w], out[b] = sd[w].clone(), sd[b].clone()
        out[w][:d] *= lam
        out[b][:d] *= lam
    return out


def image_names():
    return [(f"trunk.blocks.{i}.attn.qkv.weight", f"trunk.blocks.{i}.attn.qkv.bias") for i in range(DEPTH)]


def text_names():
    return [(f"text.transformer.resblocks.{i}.attn.in_proj_weight", f"text.transformer.resblocks.{i}.attn.in_proj_bias") for i in range(DEPTH)]


@pytest.fixture(scope="module")
def ref():
    from oracle import siglip_ref
    return siglip_ref


def round_qkv(_, qkv):
    return qkv.to(torch.bfloat16).float()


class Events:
    """qkv hook of the oracle: the share of query rows (every block, image, head) whose lazy maximum would be raised after the first half"""

    def __init__(self):
        self.rows = self.hit = 0

    def __call__(self, _, qkv):
        l2 = (qkv[0].double() @ qkv[1].double().transpose(-1, -2)).numpy() / math.sqrt(DH) * LOG2E
        ev = vote_events(l2)
        self.rows += ev.size
        self.hit += int((ev > 0).sum())
        return qkv

    @property
    def share(self):
        return self.hit / self.rows


def test_sharpened_image_tower_is_a_fair_input(ref):
    """lambda = 8 on the CPU: rounding q, k and v to bf16 (what the engine's QKV epilogue does) alone costs the fp32 model at most 1e-4
    of cosine, and the logits are in the regime the kernel tests construct (rows that raise their maximum late)."""
    cfg = dict(ref.CONFIG, depth=DEPTH)
    sd = sharpen(ref.synthetic_weights(cfg), image_names(), 8)
    img = ref.synthetic_images(1, cfg)
    ev = Events()
    plain = ref.encode_image(img, sd, cfg, qkv_hook=ev).numpy()
    cost = 1 - cosine(plain, ref.encode_image(img, sd, cfg, qkv_hook=round_qkv).numpy())
    print("image tower, lambda 8: bf16 q / k / v cost %.3g of cosine; rows with a late raise %.3f" % (cost.max(), ev.share))
    assert cost.max() <= 1e-4
    assert ev.share >= 0.05


def sharp_text_tokens():
    """The 112 token rows of the text tower's check (tests/golden/make_siglip_sharp_texts.py: synthetic texts of more than 32 real tokens
    whose bf16 cost in the oracle is small; the choice uses the oracle alone).  Batch 3 is their head."""
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "siglip_sharp_texts.npz"))["tokens"].astype(np.int64))


def test_sharpened_text_tower_is_a_fair_input(ref):
    """The same two conditions over ALL the texts the engine test runs: at least 5 % of the query rows raise their maximum late at
    lambda = 8 (so the issue's fall-back to lambda = 16 for this tower is not used), and rounding q, k, v to bf16 costs at most 1e-4.
    Plain synthetic_tokens fails the second (its first 112 texts: median 4.6e-5, 15 above 1e-4, largest 2.2e-4 -- one position of a
    64-key softmax is read, nothing averages a flipped near-tie away) and reaches the first only barely (0.052: texts that end before
    key 32 have only pad copies in their second half); hence the chosen texts."""
    cfg = dict(ref.TEXT_CONFIG, layers=DEPTH)
    sd = sharpen(ref.synthetic_text_weights(cfg), text_names(), TEXT_LAMBDA)
    tok = sharp_text_tokens()
    assert tok.shape == (max(TEXT_BATCHES), cfg["context_length"]) and int((tok != 1).sum(1).min()) > HALF
    ev = Events()
    plain = ref.encode_text(tok, sd, cfg, qkv_hook=ev).numpy()
    cost = 1 - cosine(plain, ref.encode_text(tok, sd, cfg, qkv_hook=round_qkv).numpy())
    print("text tower, lambda %d: bf16 q / k / v cost of cosine: median %.3g, largest %.3g, texts above 1e-4: %d of %d; rows with a late raise %.3f" %
          (TEXT_LAMBDA, np.median(cost), cost.max(), int((cost > 1e-4).sum()), len(cost), ev.share))
    assert ev.share >= 0.05
    assert cost.max() <= 1e-4, cost.max()


@pytest.fixture(scope="module")
def sharp_images(gpu, mse, ref):
    """per lambda: (engine, oracle rows of the largest batch)"""
    from mse import siglip
    cfg = dict(ref.CONFIG, depth=DEPTH)
    base = ref.synthetic_weights(cfg)
    img = ref.synthetic_images(max(IMAGE_BATCHES), cfg)
    out = {}
    for lam in (8, 16):
        sd = sharpen(base, image_names(), lam)
        eng = siglip.SiglipImageEngine.from_state_dict({"visual." + k: v for k, v in sd.items()}, dict(siglip.SO400M_384, depth=DEPTH),
                                                       max_batch=max(IMAGE_BATCHES))
        out[lam] = (eng, ref.encode_image(img, sd, cfg).numpy())
    yield img.numpy(), out
    for eng, _ in out.values():
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", IMAGE_BATCHES)
def test_image_tower_with_sharp_attention(sharp_images, batch):
    """Cosine within 1e-3 of the fp32 model (the project's tolerance, BASELINE.json) at lambda = 8; lambda = 16 is printed, not asserted."""
    img, engines = sharp_images
    cos = {lam: cosine(eng.encode_image(img[:batch]), want[:batch]) for lam, (eng, want) in engines.items()}
    print("image tower, batch %d: worst 1 - cosine at lambda 8: %.3g, at lambda 16: %.3g" % (batch, (1 - cos[8]).max(), (1 - cos[16]).max()))
    assert np.all(cos[8] > 1 - 1e-3), cos[8]


@pytest.fixture(scope="module")
def sharp_texts(gpu, mse, ref):
    from mse import siglip
    cfg = dict(ref.TEXT_CONFIG, layers=DEPTH)
    base = ref.synthetic_text_weights(cfg)
    tok = sharp_text_tokens()
    out = {}
    for lam in (TEXT_LAMBDA, 16):
        sd = sharpen(base, text_names(), lam)
        eng = siglip.SiglipTextEngine.from_state_dict(sd, dict(siglip.SO400M_TEXT, layers=DEPTH), max_batch=max(TEXT_BATCHES))
        out[lam] = (eng, ref.encode_text(tok, sd, cfg).numpy())
    yield tok.numpy(), out
    for eng, _ in out.values():
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", TEXT_BATCHES)
def test_text_tower_with_sharp_attention(sharp_texts, batch):
    tok, engines = sharp_texts
    cos = {lam: cosine(eng.encode_text(tok[:batch]), want[:batch]) for lam, (eng, want) in engines.items()}
    print("text tower, batch %d: worst 1 - cosine at lambda %d: %.3g, at lambda 16: %.3g" %
          (batch, TEXT_LAMBDA, (1 - cos[TEXT_LAMBDA]).max(), (1 - cos[16]).max()))
    assert np.all(cos[TEXT_LAMBDA] > 1 - 1e-3), cos[TEXT_LAMBDA]
