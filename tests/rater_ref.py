"""numpy restatement of csrc/rater.hip and csrc/rater_math.h: the ensemble rater of the reference's meme-rater/ (model.py, train.py:63-71,
active_learning.py:50-53, ensemble_to_wide_model.py:44-55) in the device's own arithmetic, on describe_ref.fma32 and
sae_train_ref.adamw32.  tests/test_rater_host.py holds it to float64 torch on the CPU; tests/test_gpu_rater.py holds the device to it,
bit for bit.

The rule, as the header of csrc/rater.hip states it (M members, E = d_emb, C channels, B pairs per member and step, R = 2 B slots: slot
2 b is pair b's first row, slot 2 b + 1 its second; f32 parameters up [M E][E], bias [M E], down [C][M E], member m owning hidden units
m E .. (m + 1) E, each with moments m and v; one step count t):
  exp_fixed   x clamped to [-87, 87]; n = rint(x * LOG2E); r = fma(n, -LN2_LO, fma(n, -LN2_HI, x)); the degree-7 Taylor polynomial by
              Horner in fma; times 2^n, exact.  sig(t) = 1 / (1 + exp_fixed(-t)); silu(u) = u * sig(u);
              silu'(u) = s * (1 + u * (1 - s)), s = sig(u), a subtract, a multiply, an add, a multiply
  forward     u = (the k-ascending fma chain from +0 of up[m E + j][k] x[k]) + bias[m E + j];  h = silu(u)
  scores      s[m][r][c]: 64 lanes, lane l the chain fma(h[j], down[c][m E + j], S_l) over j = l, l + 64, ... from +0, then the tree
              S_l += S_{l + o}, o = 32 .. 1 (sae_train_ref.hidden_dot)
  head        z = s[2b] - s[2b+1]; p = sig(z); g = (p - y) * invN, invN = (float)(1.0 / (double)(M B C))
  loss        per element -(y lp + (1 - y) lq), lp = log(p), lq = log(1 - p) in f64 from the f32 p, each raised to -100 where below;
              summed over (m, b, c) ascending from +0, divided by M B C
  gate        a non-finite row in a slot or a non-finite loss: the step is refused and changes nothing
  backward    ds[r][c] = g[r / 2][c], negated for odd r; g_down[c][m E + j] = fma(ds[r][c], h[r][j], G) over r ascending from +0;
              dh[r][j] = fma(ds[r][c], down[c][m E + j], D) over c ascending from +0; du = dh * silu'(u);
              g_bias[m E + j] = G + du[r][j] over r ascending; g_up[m E + j][k] = fma(du[r][j], x[r][k], G) over r ascending from +0
  AdamW       sae_train_ref.adamw32
  variance    p_m = sig(s[a][m][c] - s[b][m][c]); mean = (sum over m ascending from +0) / f32(M); var = (sum of (p_m - mean)^2 the same
              way) / f32(M - 1); the largest over c"""
import math

import numpy as np

import sae_train_ref
from describe_ref import fma32
from sae_train_ref import U, adamw32, gamma  # noqa: F401

EXP_LO, EXP_HI = np.float32(-87.0), np.float32(87.0)


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


LOG2E, LN2_HI, LN2_LO = _f(0x3FB8AA3B), _f(0x3F317200), _f(0x35BFBE8E)
# 1 / k! for k = 7 .. 2, each rounded to f32 once
COEFFS = tuple(np.float32(1.0 / math.factorial(k)) for k in range(7, 1, -1))
# the largest error of exp_fixed in f32 ulps against float64 numpy.exp over test_rater_host.py's sweep (0.914 measured), rounded up
EXP_ULPS = 1


def exp_fixed(x):
    """rater_math.h's exp_fixed on an f32 array, bit for bit"""
    x = np.asarray(x, np.float32)
    shape, x = x.shape, x.reshape(-1)                          # fma32 takes no 0-d array
    with np.errstate(invalid="ignore"):
        x = np.where(x < EXP_LO, EXP_LO, x)
        x = np.where(x > EXP_HI, EXP_HI, x).astype(np.float32)
        n = np.rint((x * LOG2E).astype(np.float32)).astype(np.float32)
        r = fma32(n, -LN2_HI, x)
        r = fma32(n, -LN2_LO, r)
        p = np.full(x.shape, COEFFS[0], np.float32)
        for c in COEFFS[1:]:
            p = fma32(p, r, c)
        p = fma32(p, r, np.float32(1.0))
        p = fma32(p, r, np.float32(1.0))
        nan = np.isnan(n)
        scale = ((np.where(nan, 0, n).astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
        return np.where(nan, n, (p * scale).astype(np.float32)).astype(np.float32).reshape(shape)


def sig(t):
    t = np.asarray(t, np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + exp_fixed(-t))).astype(np.float32)


def silu(u):
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (u * sig(u)).astype(np.float32)


def silu_grad(u):
    u = np.asarray(u, np.float32)
    s = sig(u)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.float32(1.0) - s).astype(np.float32)
        b = (u * a).astype(np.float32)
        c = (np.float32(1.0) + b).astype(np.float32)
        return (s * c).astype(np.float32)


def map_rating(rating):
    """shared.py:23-38"""
    table = {"1": 0.9, "2": 0.1, "2+": 0.3, "2p": 0.3, "1+": 0.7, "1p": 0.7, "eq": 0.5}
    return np.array([table[r] for r in rating.split(",")])


class Model:
    """The parameters and the optimizer state of one run, in the wide layout; arrays are float32."""

    def __init__(self, up, bias, down, n_members, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.up, self.bias, self.down = np.array(up, np.float32), np.array(bias, np.float32), np.array(down, np.float32)
        self.M, self.E, self.C = int(n_members), self.up.shape[1], self.down.shape[0]
        assert self.up.shape == (self.M * self.E, self.E) and self.bias.shape == (self.M * self.E,) and self.down.shape == (self.C, self.M * self.E)
        self.lr, self.betas, self.eps, self.wd = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.t = 0
        self.m = {k: np.zeros_like(v) for k, v in self.params().items()}
        self.v = {k: np.zeros_like(v) for k, v in self.params().items()}

    def params(self):
        return {"up": self.up, "bias": self.bias, "down": self.down}

    def state(self):
        """the layout of RaterTrainer.state()"""
        out = {"t": self.t}
        for name, arr in (("m", self.m), ("v", self.v)):
            for k in ("up", "bias", "down"):
                out[name + "_" + k] = arr[k]
        return out


def random_weights(E, M, C, rng):
    """nn.Linear's default distribution (both layers have fan-in E) from a numpy Generator, in the wide layout -> (up, bias, down)"""
    b = 1.0 / math.sqrt(E)
    up = rng.uniform(-b, b, (M * E, E)).astype(np.float32)
    bias = rng.uniform(-b, b, M * E).astype(np.float32)
    down = rng.uniform(-b, b, (C, M * E)).astype(np.float32)
    return up, bias, down


def hidden(model, x):
    """u, h [M, R, E] of the slots x [M, R, E] f32 (the exact widening of the f16 rows)"""
    M, E = model.M, model.E
    x = np.asarray(x, np.float32)
    up = model.up.reshape(M, 1, E, E)
    a = np.zeros((M, x.shape[1], E), np.float32)
    for k in range(E):
        a = fma32(up[:, :, :, k], x[:, :, k:k + 1], a)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (a + model.bias.reshape(M, 1, E)).astype(np.float32)
    return u, silu(u)


def scores_of(model, h):
    """s [M, R, C] from h [M, R, E]"""
    M, E, C = model.M, model.E, model.C
    R = h.shape[1]
    s = np.empty((M, R, C), np.float32)
    for c in range(C):
        w = np.broadcast_to(model.down[c].reshape(M, 1, E), (M, R, E)).reshape(M * R, E)
        s[:, :, c] = sae_train_ref.hidden_dot(h.reshape(M * R, E), w).reshape(M, R)
    return s


def member_scores(model, x):
    """[n, M, C]: every member's scores of the rows x [n, E] f32"""
    x = np.asarray(x, np.float32)
    _, h = hidden(model, np.broadcast_to(x[None], (model.M,) + x.shape))
    return np.ascontiguousarray(scores_of(model, h).transpose(1, 0, 2))


def head(s, y):
    """(p [M, B, C] f32, loss f64) of the slot scores s [M, 2 B, C] under targets y [M, B, C] f32"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = (s[:, 0::2] - s[:, 1::2]).astype(np.float32)
        p = sig(z)
        pd, yd = p.astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
        lp, lq = np.log(pd), np.log(1.0 - pd)
        lp, lq = np.where(lp < -100.0, -100.0, lp), np.where(lq < -100.0, -100.0, lq)
        terms = -(yd * lp + (1.0 - yd) * lq)
        total = 0.0
        for t in terms.reshape(-1):
            total = total + float(t)
    return p, total / float(terms.size)


def gradients(model, x, y):
    """The forward and backward pass; x [M, 2 B, E] f32 slots, y [M, B, C] f32 -> None where the step is refused, else
    (loss, {up, bias, down}, s [M, 2 B, C])."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    M, E, C = model.M, model.E, model.C
    R = x.shape[1]
    B = R // 2
    if not np.isfinite(x).all():
        return None
    u, h = hidden(model, x)
    s = scores_of(model, h)
    p, loss = head(s, y)
    if not math.isfinite(loss):
        return None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        g = ((p - y).astype(np.float32) * np.float32(1.0 / float(M * B * C))).astype(np.float32)
        ds = np.empty((M, R, C), np.float32)
        ds[:, 0::2], ds[:, 1::2] = g, -g
        down = model.down.reshape(C, M, E)
        g_down = np.zeros((C, M, E), np.float32)
        for r in range(R):
            g_down = fma32(ds[:, r, :].T[:, :, None], h[None, :, r, :], g_down)
        dh = np.zeros((M, R, E), np.float32)
        for c in range(C):
            dh = fma32(ds[:, :, c:c + 1], down[c][:, None, :], dh)
        du = (dh * silu_grad(u)).astype(np.float32)
        g_bias = np.zeros((M, E), np.float32)
        g_up = np.zeros((M, E, E), np.float32)
        for r in range(R):
            g_bias = (g_bias + du[:, r]).astype(np.float32)
            g_up = fma32(du[:, r, :, None], x[:, r, None, :], g_up)
    return loss, {"up": g_up.reshape(M * E, E), "bias": g_bias.reshape(M * E), "down": g_down.reshape(C, M * E)}, s


def step(model, x, y):
    """One training step in place; -> the loss, or None where the step is refused (nothing changes)"""
    got = gradients(model, x, y)
    if got is None:
        return None
    loss, g, _ = got
    model.t += 1
    for name, p in model.params().items():
        p[...], model.m[name][...], model.v[name][...] = adamw32(p, model.m[name], model.v[name], g[name], model.t, model.lr, model.betas,
                                                                 model.eps, model.wd)
    return loss


def slots_of(rows_f32, pair_ids):
    """x [M, 2 B, E] of one step's pair ids [M, B, 2] into rows_f32 [n, E]"""
    ids = np.asarray(pair_ids, np.int64)
    return rows_f32[ids.reshape(ids.shape[0], -1)]


def pair_variance(table, a, b):
    """[n_pairs] f32 from a member-score table [n, M, C]"""
    table = np.asarray(table, np.float32)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    M = table.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        p = sig((table[a] - table[b]).astype(np.float32))          # [n_pairs, M, C]
        total = np.zeros((p.shape[0], p.shape[2]), np.float32)
        for m in range(M):
            total = (total + p[:, m]).astype(np.float32)
        mean = (total / np.float32(M)).astype(np.float32)
        acc = np.zeros_like(total)
        for m in range(M):
            d = (p[:, m] - mean).astype(np.float32)
            acc = (acc + (d * d).astype(np.float32)).astype(np.float32)
        var = (acc / np.float32(M - 1)).astype(np.float32)
        best = var[:, 0]
        for c in range(1, var.shape[1]):
            best = np.where(var[:, c] > best, var[:, c], best)
    return best.astype(np.float32)


def top_pairs(variances, k):
    """indices of the k pairs of largest variance: variance descending, pair index ascending"""
    v = np.asarray(variances, np.float32)
    return np.array(sorted(range(v.size), key=lambda i: (-float(v[i]), i))[:k], np.int64)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------
def gradients64(up, bias, down, M, x, y):
    """The same step in plain float64 (any summation order), the closed-form head -> (loss, {up, bias, down}, z [M, B, C])"""
    up, bias, down, x, y = (np.asarray(a, np.float64) for a in (up, bias, down, x, y))
    E, C = up.shape[1], down.shape[0]
    R = x.shape[1]
    B = R // 2
    upm, bm, dm = up.reshape(M, E, E), bias.reshape(M, E), down.reshape(C, M, E)
    u = np.einsum("mjk,mrk->mrj", upm, x) + bm[:, None, :]
    sg = 1.0 / (1.0 + np.exp(-u))
    h = u * sg
    s = np.einsum("mrj,cmj->mrc", h, dm)
    z = s[:, 0::2] - s[:, 1::2]
    p = 1.0 / (1.0 + np.exp(-z))
    loss = float(-(y * np.log(p) + (1 - y) * np.log1p(-p)).mean())
    g = (p - y) / (M * B * C)
    ds = np.empty((M, R, C))
    ds[:, 0::2], ds[:, 1::2] = g, -g
    dh = np.einsum("mrc,cmj->mrj", ds, dm)
    du = dh * (sg * (1 + u * (1 - sg)))
    grads = {"down": np.einsum("mrc,mrj->cmj", ds, h).reshape(C, M * E), "bias": du.sum(axis=1).reshape(M * E),
             "up": np.einsum("mrj,mrk->mjk", du, x).reshape(M * E, E)}
    return loss, grads, z


def gradient_bounds(up, bias, down, M, x, y):
    """Bounds on |f32 restatement - float64| for the loss and every gradient.  u = 2^-24, gamma_n = n u / (1 - n u) bounds a chain or tree
    of n roundings (Higham, Accuracy and Stability, 3.1-3.4); e = EXP_ULPS.  Each line takes the line before as its input error (x' means
    |x| + dx):
      u     gamma_E sum_k |up_jk| |x_k| + U |u|                                     the fma chain and the bias add
      sig   sig(t) of an input off by dt: (2 e + 3) U sig + dt / 4                   exp within e ulps (2 e U relative), the add, the divide;
                                                                                    |sig'| <= 1/4
      h     du sig' + |u| dsig + U |h|'                                             one multiply; d silu / du = silu' is bounded by 1.1
      s     gamma_(E/64 + 7) sum_j h' |down| + sum_j dh |down|                       chains of ceil(E / 64) and a tree of 6, any order
      z     ds_a + ds_b + U |z|;   p: sig's line;   g: (dp + U (|p - y| + dp)) invN (1 + 3 U)   the subtract, invN's rounding, the multiply
      loss  mean of dp (y / p + (1 - y) / (1 - p)) (1 + 1e-9) + 1e-14 L             log's derivative at p, second order covered by 1e-9
      g_dn  gamma_R sum_r g' h' + sum_r (dg |h| + |g| dh)
      dh    gamma_C sum_c g' |down| + sum_c dg |down|
      silu' s (1 + u (1 - s)): dsig (1 + 2 |u|) + du / 4 + 4 U (1 + |u|)             sig enters twice; s (1 - s) <= 1/4; four roundings
      du    ddh |silu'|' + |dh| dsilu' + U |du|'
      g_b   gamma_R sum_r du' + sum_r ddu;   g_up  gamma_R sum_r du' |x| + sum_r ddu |x|"""
    up64, b64, down64, x64, y64 = (np.asarray(a, np.float64) for a in (up, bias, down, x, y))
    E, C = up64.shape[1], down64.shape[0]
    R = x64.shape[1]
    B = R // 2
    e = EXP_ULPS
    upm, dm = up64.reshape(M, E, E), down64.reshape(C, M, E)
    u = np.einsum("mjk,mrk->mrj", upm, x64) + b64.reshape(M, 1, E)
    d_u = gamma(E) * np.einsum("mjk,mrk->mrj", np.abs(upm), np.abs(x64)) + U * np.abs(u)

    def sig_err(t, dt):
        s = 1.0 / (1.0 + np.exp(-t))
        return s, (2 * e + 3) * U * s + dt / 4

    sg, d_sg = sig_err(u, d_u)
    h = u * sg
    d_h = d_u * 1.1 + np.abs(u) * d_sg + U * (np.abs(h) + d_u * 1.1 + np.abs(u) * d_sg)
    h1 = np.abs(h) + d_h
    s = np.einsum("mrj,cmj->mrc", h, dm)
    d_s = gamma(-(-E // 64) + 7) * np.einsum("mrj,cmj->mrc", h1, np.abs(dm)) + np.einsum("mrj,cmj->mrc", d_h, np.abs(dm))
    z = s[:, 0::2] - s[:, 1::2]
    d_z = d_s[:, 0::2] + d_s[:, 1::2]
    d_z = d_z + U * (np.abs(z) + d_z)
    p, d_p = sig_err(z, d_z)
    inv_n = 1.0 / (M * B * C)
    g = (p - y64) * inv_n
    d_g = (d_p + U * (np.abs(p - y64) + d_p)) * inv_n * (1 + 3 * U)
    g1 = np.abs(g) + d_g
    L = float(-(y64 * np.log(p) + (1 - y64) * np.log1p(-p)).mean())
    d_L = float((d_p * (y64 / p + (1 - y64) / (1 - p))).mean() * (1 + 1e-9) + 1e-14 * abs(L))
    rep = lambda a: np.repeat(a, 2, axis=1)                        # [M, B, C] -> [M, R, C]
    ga, dga, g1a = rep(np.abs(g)), rep(d_g), rep(g1)
    bounds = {"down": (gamma(R) * np.einsum("mrc,mrj->cmj", g1a, h1) + np.einsum("mrc,mrj->cmj", dga, np.abs(h)) +
                       np.einsum("mrc,mrj->cmj", ga, d_h)).reshape(C, M * E)}
    ds = np.empty((M, R, C))
    ds[:, 0::2], ds[:, 1::2] = g, -g
    dh = np.einsum("mrc,cmj->mrj", ds, dm)
    d_dh = gamma(C) * np.einsum("mrc,cmj->mrj", g1a, np.abs(dm)) + np.einsum("mrc,cmj->mrj", dga, np.abs(dm))
    sp = sg * (1 + u * (1 - sg))
    d_sp = d_sg * (1 + 2 * np.abs(u)) + 0.25 * d_u + 4 * U * (1 + np.abs(u))
    du = dh * sp
    d_du = d_dh * (np.abs(sp) + d_sp) + np.abs(dh) * d_sp
    d_du = d_du + U * (np.abs(du) + d_du)
    du1 = np.abs(du) + d_du
    bounds["bias"] = (gamma(R) * du1.sum(axis=1) + d_du.sum(axis=1)).reshape(M * E)
    bounds["up"] = (gamma(R) * np.einsum("mrj,mrk->mjk", du1, np.abs(x64)) + np.einsum("mrj,mrk->mjk", d_du, np.abs(x64))).reshape(M * E, E)
    return d_L, bounds, z


# ---- the planted utility of the end-to-end tests -------------------------------------------------------------------------------------------
PLANTED = dict(E=32, M=4, C=1, B=1, seed=5, lr=2e-3, steps=300, n_train_rows=300, n_rows=400, n_pairs=150, n_held_out=256)
_planted = {}


def planted_case():
    """A hidden direction w in E = 32: rows, 150 rated training pairs among the first 300 rows, 256 held-out pairs among the last 100,
    ratings 0.9 / 0.1 by the sign of the utility difference, a fresh ensemble, and the pair ids of every step (each member its own
    permutation per epoch, batch 1) -> dict"""
    if "case" not in _planted:
        P = PLANTED
        rng = np.random.default_rng(P["seed"])
        rows = rng.standard_normal((P["n_rows"], P["E"])).astype(np.float16)
        utility = rows.astype(np.float64) @ rng.standard_normal(P["E"])

        def rated(lo, hi, n):
            a, b = rng.integers(lo, hi, n), rng.integers(lo, hi, n)
            b = np.where(a == b, lo + (b - lo + 1) % (hi - lo), b)
            return np.stack([a, b], axis=1).astype(np.uint32), np.where(utility[a] > utility[b], 0.9, 0.1).astype(np.float32)[:, None]

        pairs, ratings = rated(0, P["n_train_rows"], P["n_pairs"])
        held, held_ratings = rated(P["n_train_rows"], P["n_rows"], P["n_held_out"])
        up, bias, down = random_weights(P["E"], P["M"], P["C"], rng)
        orders = []
        while len(orders) * P["n_pairs"] < P["steps"]:
            orders.append(np.stack([rng.permutation(P["n_pairs"]) for _ in range(P["M"])]))       # [M, n_pairs] per epoch
        order = np.concatenate(orders, axis=1)[:, :P["steps"]].T                                     # [steps, M]
        _planted["case"] = dict(rows=rows.view(np.uint16), pairs=pairs, ratings=ratings, held=held, held_ratings=held_ratings, up=up, bias=bias,
                                down=down, pair_ids=pairs[order][:, :, None, :], targets=ratings[order][:, :, None, :])
    return _planted["case"]


def evaluate(model, rows_f32, pairs, ratings):
    """(mean BCE over members and pairs in float64, share of pairs the mean member score orders as rated) -- train.py:85-95's evaluation"""
    pairs = np.asarray(pairs, np.int64)
    s = member_scores(model, rows_f32)[:, :, 0]                                                     # [n, M]
    z = (s[pairs[:, 0]] - s[pairs[:, 1]]).astype(np.float32)
    p = sig(z).astype(np.float64)
    y = np.asarray(ratings, np.float64)[:, :1]
    loss = float(-(y * np.log(p) + (1 - y) * np.log1p(-p)).mean())
    return loss, float(((z.astype(np.float64).mean(axis=1) > 0) == (y[:, 0] > 0.5)).mean())


def planted_run():
    """((loss, share) before, (loss, share) after, the trained Model) of the restated run, computed once"""
    if "run" not in _planted:
        c, P = planted_case(), PLANTED
        rows = c["rows"].view(np.float16).astype(np.float32)
        model = Model(c["up"], c["bias"], c["down"], P["M"], lr=P["lr"])
        before = evaluate(model, rows, c["held"], c["held_ratings"])
        for s in range(P["steps"]):
            assert step(model, slots_of(rows, c["pair_ids"][s]), c["targets"][s]) is not None
        _planted["run"] = (before, evaluate(model, rows, c["held"], c["held_ratings"]), model)
    return _planted["run"]
