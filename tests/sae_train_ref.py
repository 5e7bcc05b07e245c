"""numpy restatement of csrc/sae_train.hip: one training step of the reference's sparse autoencoder (sae/train.py:51-59: F.mse_loss,
backward, torch.optim.AdamW) in the device's own arithmetic, on describe_ref.fma32 and sae_ref.  tests/test_sae_train_host.py holds it
to a float64 torch module and to torch.optim.AdamW on the CPU; tests/test_gpu_sae_train.py holds the device to it, bit for bit.

The rule, as the header of csrc/sae_train.hip states it (B rows, E = d_emb, H = d_hidden, K = top_k; f32 parameters up [H][E], up_bias
[H] optional, downT [H][E], down_bias [E], each with moments m and v; one step count t):
  forward     sae_ref: counts, canonical features, activations a, reconstruction r, the f64 squared error of every row
  gate        an invalid (NaN) row or a non-finite loss: the step is refused and changes nothing
  loss        L = (sum of sqerr_i, i ascending from +0, f64) / (double)(B E)
  gR          e = f32(r - x); gR[i][d] = e * s, one f32 multiply, s = (float)(2.0 / (double)(B E))
  pairs       the kept (i, f), grouped by feature, members in ascending i
  hidden      h = sum_d downT[f][d] gR[i][d], weights from before the update: 64 lanes, lane l the fma chain over d = l, l + 64, ... from
              +0, then the tree S_l += S_{l + o}, o = 32 .. 1
  gradients   chains from +0 over a feature's members, i ascending: g_up[f][k] = fma(h, x[i][k], g); g_downT[f][d] = fma(a, gR[i][d], g);
              g_up_bias[f] = g + h; g_down_bias[d] = g + gR[i][d] over all rows.  No members: +0
  AdamW       p = p decay; m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g; p = p - step_size (m / (sqrt(v) / bc2_sqrt + eps)), every
              operation one f32 rounding; decay = (float)(1 - lr wd), step_size = (float)(lr / (1 - b1^t)),
              bc2_sqrt = (float)sqrt(1 - b2^t) from doubles
  counters    a completed step adds one per pair to its feature's counter"""
import math

import numpy as np

import sae_ref
from describe_ref import fma32

LANES = 64
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


class Model:
    """The parameters, the optimizer state and the counters of one run; arrays are float32, down in the checkpoint's layout."""

    def __init__(self, up, down, up_bias, down_bias, top_k, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.up = np.array(up, np.float32)
        self.down_t = np.array(np.asarray(down, np.float32).T, order="C")   # a copy always: the steps update it in place
        self.up_bias = None if up_bias is None else np.array(up_bias, np.float32)
        self.down_bias = np.array(down_bias, np.float32)
        self.top_k, self.lr, self.betas, self.eps, self.wd = top_k, float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.t = 0
        self.m = {k: np.zeros_like(v) for k, v in self.params().items()}
        self.v = {k: np.zeros_like(v) for k, v in self.params().items()}
        self.counters = np.zeros(self.up.shape[0], np.uint64)

    def params(self):
        p = {"up": self.up, "down_t": self.down_t, "down_bias": self.down_bias}
        if self.up_bias is not None:
            p["up_bias"] = self.up_bias
        return p

    @property
    def down(self):
        return np.array(self.down_t.T, order="C")

    def state(self):
        """the layout of SaeTrainer.state()"""
        out = {"t": self.t}
        for name, arr in (("m", self.m), ("v", self.v)):
            out[name + "_up"], out[name + "_down"], out[name + "_down_bias"] = arr["up"], np.ascontiguousarray(arr["down_t"].T), arr["down_bias"]
            if self.up_bias is not None:
                out[name + "_up_bias"] = arr["up_bias"]
        return out


def hidden_dot(w, g):
    """[P] f32: the 64-lane chains and the tree over rows of w and g, [P, E]"""
    P, E = w.shape
    S = np.zeros((P, LANES), np.float32)
    for j in range(-(-E // LANES)):
        lanes = min(LANES, E - j * LANES)
        S[:, :lanes] = fma32(w[:, j * LANES:j * LANES + lanes], g[:, j * LANES:j * LANES + lanes], S[:, :lanes])
    o = LANES // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while o:
            S[:, :o] = S[:, :o] + S[:, o:2 * o]
            o //= 2
    return S[:, 0].copy()


def pair_index(counts, feats, acts):
    """(rows, features, activations, level) of the kept pairs in (feature, row) order; level = the pair's place among its feature's"""
    rows = np.concatenate([np.full(int(c), i, np.int64) for i, c in enumerate(counts)] or [np.zeros(0, np.int64)])
    fs = np.concatenate([feats[i, :int(c)].astype(np.int64) for i, c in enumerate(counts)] or [np.zeros(0, np.int64)])
    a = np.concatenate([acts[i, :int(c)] for i, c in enumerate(counts)] or [np.zeros(0, np.float32)]).astype(np.float32)
    order = np.lexsort((rows, fs))
    rows, fs, a = rows[order], fs[order], a[order]
    level = np.zeros(rows.size, np.int64)
    for p in range(1, rows.size):
        level[p] = level[p - 1] + 1 if fs[p] == fs[p - 1] else 0
    return rows, fs, a, level


def gradients(model, x):
    """The forward and backward pass in the device's arithmetic; x [B, E] f32 (the exact widening of the f16 rows).
    -> None where the step is refused, else (loss, grads {name: f32 array}, (pair rows, pair features))."""
    x = np.asarray(x, np.float32)
    B, E = x.shape
    H = model.up.shape[0]
    counts, feats, acts = sae_ref.encode(model.up, x, model.top_k, model.up_bias)
    if (counts == sae_ref.NONE).any():
        return None
    r = sae_ref.reconstruct(model.down, model.down_bias, counts, feats, acts)
    sq = sae_ref.sq_errors(r, x)
    total = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for s in sq:
            total = total + float(s)
    loss = total / float(B * E)
    if not math.isfinite(loss):
        return None
    with np.errstate(invalid="ignore", over="ignore"):
        e = (r - x).astype(np.float32)
        gR = (e * np.float32(2.0 / float(B * E))).astype(np.float32)
        rows, fs, a, level = pair_index(counts, feats, acts)
        h = hidden_dot(model.down_t[fs], gR[rows])
        g = {"up": np.zeros((H, E), np.float32), "down_t": np.zeros((H, E), np.float32), "down_bias": np.zeros(E, np.float32)}
        g_ub = np.zeros(H, np.float32)
        for lv in range(int(level.max()) + 1 if level.size else 0):
            on = np.nonzero(level == lv)[0]
            f, i = fs[on], rows[on]
            g["up"][f] = fma32(h[on][:, None], x[i], g["up"][f])
            g["down_t"][f] = fma32(a[on][:, None], gR[i], g["down_t"][f])
            g_ub[f] = g_ub[f] + h[on]
        for i in range(B):
            g["down_bias"] = (g["down_bias"] + gR[i]).astype(np.float32)
    if model.up_bias is not None:
        g["up_bias"] = g_ub
    return loss, g, (rows, fs)


def adam_constants(lr, wd, betas, t):
    """(decay, step_size, bc2_sqrt) of step number t, float32 from doubles"""
    return (np.float32(1.0 - lr * wd), np.float32(lr / (1.0 - betas[0] ** t)), np.float32(math.sqrt(1.0 - betas[1] ** t)))


def adamw32(p, m, v, g, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """One AdamW step, number t, elementwise in float32 in the stated operation order -> (p, m, v)"""
    decay, step_size, bc2_sqrt = adam_constants(lr, wd, betas, t)
    b1, b2, eps, one = np.float32(betas[0]), np.float32(betas[1]), np.float32(eps), np.float32(1.0)
    p, m, v, g = (np.asarray(z, np.float32) for z in (p, m, v, g))
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        p = p * decay
        m = b1 * m + (one - b1) * g
        v = b2 * v + ((one - b2) * g) * g
        p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + eps))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adamw64(p, m, v, g, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """torch.optim.AdamW's step number t in float64 -> (p, m, v)"""
    p, m, v, g = (np.asarray(z, np.float64) for z in (p, m, v, g))
    p = p * (1.0 - lr * wd)
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    p = p - (lr / (1 - betas[0] ** t)) * m / (np.sqrt(v) / math.sqrt(1 - betas[1] ** t) + eps)
    return p, m, v


def step(model, x):
    """One training step in place; -> the loss, or None where the step is refused (nothing changes)"""
    got = gradients(model, x)
    if got is None:
        return None
    loss, g, (_, fs) = got
    model.t += 1
    for name, p in model.params().items():
        p[...], model.m[name][...], model.v[name][...] = adamw32(p, model.m[name], model.v[name], g[name], model.t, model.lr, model.betas,
                                                                 model.eps, model.wd)
    model.counters += np.bincount(fs, minlength=model.up.shape[0]).astype(np.uint64)
    return loss


def train(model, x, batch):
    """steps over consecutive batches of x until one is refused -> the losses of the completed steps"""
    losses = []
    for s in range(x.shape[0] // batch):
        loss = step(model, x[s * batch:(s + 1) * batch])
        if loss is None:
            break
        losses.append(loss)
    return np.array(losses, np.float64)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------
def gradients64(up, up_bias, down, down_bias, x, top_k):
    """The same step in plain float64 (dense, any summation order) -> (loss, {up, down [E, H], down_bias, up_bias}, mask, z, a)"""
    up, down, down_bias, x = (np.asarray(z, np.float64) for z in (up, down, down_bias, x))
    B, E = x.shape
    z = x @ up.T + (0.0 if up_bias is None else np.asarray(up_bias, np.float64)[None, :])
    act = np.maximum(z, 0.0)
    t = np.sort(act, axis=1)[:, act.shape[1] - top_k - 1]
    mask = act > t[:, None]
    a = np.where(mask, act, 0.0)
    e = a @ down.T + down_bias - x
    gR = e * (2.0 / (B * E))
    h = (gR @ down) * mask
    return float((e * e).sum() / (B * E)), {"up": h.T @ x, "down": gR.T @ a, "down_bias": gR.sum(axis=0), "up_bias": h.sum(axis=0)}, mask, z, a


def gradient_bounds(up, up_bias, down, down_bias, x, top_k):
    """Bounds on |f32 restatement - float64| for the loss and every gradient, where both keep the same features (the caller asserts the
    selection margin).  u = 2^-24, gamma_n = n u / (1 - n u) bounds a chain or tree of n roundings (Higham, Accuracy and Stability,
    3.1-3.4).  Each line takes the line before as its input error:
      a     gamma_E sum_k |up_jk| |x_k| + u |z_j|                        the fma chain and the bias add (sae.hip's B_j)
      r     gamma_c (sum_f a' |down_df| + |bias_d|) + sum_f da_f |down_df|   c = the row's kept features, a' = |a| + da
      e     dr + u (|e| + dr)                                             one subtraction
      gR    s (de + 2 u (|e| + de)) (1 + 3 u)                             the rounding of s and one multiply
      L     sum_i,d de (2 |e| + de) / (B E) + 1e-14 L                      squares and sums in f64
      h     gamma_E sum_d |down_df| g' + sum_d |down_df| dg              g' = |gR| + dg; a dot of E terms in any order
      g_up  gamma_n sum_i h' |x_ik| + sum_i dh |x_ik|                     n = the feature's members, h' = |h| + dh
      g_dn  gamma_n sum_i a' g' + sum_i (da g' + |a| dg)
      g_ub  gamma_n sum_i h' + sum_i dh;   g_db  gamma_B sum_i g' + sum_i dg"""
    up64, down64, x64 = (np.asarray(z, np.float64) for z in (up, down, x))
    B, E = x64.shape
    L, g, mask, z, a = gradients64(up, up_bias, down, down_bias, x, top_k)
    da = (gamma(E) * (np.abs(x64) @ np.abs(up64).T) + U * np.abs(z)) * mask
    a1 = np.abs(a) + da
    c = mask.sum(axis=1)[:, None]
    dr = gamma(c) * (a1 @ np.abs(down64).T + np.abs(np.asarray(down_bias, np.float64))[None, :]) + da @ np.abs(down64).T
    e = a @ down64.T + np.asarray(down_bias, np.float64) - x64
    de = dr + U * (np.abs(e) + dr)
    s = 2.0 / (B * E)
    dg = s * (de + 2 * U * (np.abs(e) + de)) * (1 + 3 * U)
    g1 = np.abs(e) * s + dg
    dL = float((de * (2 * np.abs(e) + de)).sum() / (B * E) + 1e-14 * L)
    h = (e * s) @ down64 * mask
    dh = (gamma(E) * (g1 @ np.abs(down64)) + dg @ np.abs(down64)) * mask
    h1 = np.abs(h) + dh
    n = mask.sum(axis=0)
    bounds = {"up": gamma(n)[:, None] * (h1.T @ np.abs(x64)) + dh.T @ np.abs(x64),
              "down": (gamma(n)[:, None] * (a1.T @ g1) + da.T @ g1 + np.abs(a).T @ dg).T,
              "up_bias": gamma(n) * h1.sum(axis=0) + dh.sum(axis=0),
              "down_bias": gamma(B) * g1.sum(axis=0) + dg.sum(axis=0)}
    return dL, bounds
