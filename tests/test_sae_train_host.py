"""CPU checks of tests/sae_train_ref.py, the restatement tests/test_gpu_sae_train.py holds the device to: its loss and gradients are
those of the reference's module (sae/model.py:31-43 under F.mse_loss, sae/train.py:55-57) written anew in float64 torch, its update is
torch.optim.AdamW, and features that tie at the threshold get no gradient."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sae_ref
import sae_train_ref as ref

SHAPES = [(8, 300, 16, 64), (33, 300, 16, 64)]   # (E, H, K, B)


@functools.lru_cache(maxsize=None)
def case(shape, seed):
    E, H, K, B = shape
    rng = np.random.default_rng(seed)
    up = (rng.uniform(-1, 1, (H, E)) / np.sqrt(E)).astype(np.float32)
    x = rng.standard_normal((B, E)).astype(np.float16).astype(np.float32)
    down = (rng.uniform(-1, 1, (E, H)) / np.sqrt(H)).astype(np.float32)
    down_bias = (rng.uniform(-1, 1, E) / np.sqrt(H)).astype(np.float32)
    return up, down, down_bias, x


def assert_selection_margin(up, x, K):
    """In float64: every row's gaps between its K-th, (K+1)-th and (K+2)-th largest activations exceed 4 max_j B_j (sae.hip's bound on
    the f32 pre-activation), so float32 and float64 keep the same features and see the same threshold."""
    up64, x64 = up.astype(np.float64), x.astype(np.float64)
    z = x64 @ up64.T
    Bj = ref.gamma(up.shape[1]) * (np.abs(x64) @ np.abs(up64).T) + ref.U * np.abs(z)
    top = -np.sort(-np.maximum(z, 0.0), axis=1)[:, K - 1:K + 2]
    gaps = np.minimum(top[:, 0] - top[:, 1], top[:, 1] - top[:, 2])
    assert (gaps > 4 * Bj.max(axis=1)).all(), "the selection margin does not hold for this draw"


def torch_gradients(up, up_bias, down, down_bias, x, K):
    """linear, relu, kthvalue(H - K), strict where, linear, mse_loss, backward: float64, on the CPU"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    W1, W2, b2, xb = t(up), t(down), t(down_bias), torch.tensor(np.asarray(x, np.float64))
    b1 = None if up_bias is None else t(up_bias)
    with torch.enable_grad():                              # other tests of the suite switch autograd off for the process
        a = F.relu(F.linear(xb, W1, b1))
        thr = torch.kthvalue(a, k=a.shape[-1] - K, dim=-1).values.unsqueeze(-1).expand_as(a)
        a = torch.where(a > thr, a, torch.zeros_like(a))
        loss = F.mse_loss(F.linear(a, W2, b2), xb)
        loss.backward()
    g = {"up": W1.grad.numpy(), "down": W2.grad.numpy(), "down_bias": b2.grad.numpy()}
    if b1 is not None:
        g["up_bias"] = b1.grad.numpy()
    return float(loss.detach()), g


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_loss_and_gradients_against_float64_torch(shape, seed):
    E, H, K, B = shape
    up, down, down_bias, x = case(shape, seed)
    assert_selection_margin(up, x, K)
    want_loss, want = torch_gradients(up, None, down, down_bias, x, K)
    # the float64 sibling: the same numbers to float64 rounding
    loss64, g64, _, _, _ = ref.gradients64(up, None, down, down_bias, x, K)
    assert abs(loss64 - want_loss) <= 1e-13 * abs(want_loss)
    for name in ("up", "down", "down_bias"):
        scale = np.abs(want[name]).max()
        assert np.abs(g64[name] - want[name]).max() <= 1e-12 * scale, name
    # the f32 restatement: within the derived bounds
    model = ref.Model(up, down, None, down_bias, K)
    loss, g, _ = ref.gradients(model, x)
    d_loss, bounds = ref.gradient_bounds(up, None, down, down_bias, x, K)
    assert abs(loss - want_loss) <= d_loss
    got = {"up": g["up"], "down": g["down_t"].T, "down_bias": g["down_bias"]}
    worst = {"loss": abs(loss - want_loss) / d_loss}
    for name in got:
        err = np.abs(got[name].astype(np.float64) - want[name])
        assert (err <= bounds[name]).all(), name
        on = bounds[name] > 0
        assert not got[name][~on].any()                   # no members: exactly zero
        worst[name] = float((err[on] / bounds[name][on]).max())
    print("sae training gradients %s seed %d: largest error / bound %s" % (shape, seed, {k: "%.3g" % v for k, v in worst.items()}))


def test_encoder_bias_gradient_against_float64_torch():
    E, H, K, B = SHAPES[1]
    up, down, down_bias, x = case(SHAPES[1], 0)
    up_bias = (np.random.default_rng(3).uniform(-1, 1, H) * 1e-3).astype(np.float32)
    want_loss, want = torch_gradients(up, up_bias, down, down_bias, x, K)
    loss64, g64, mask, _, _ = ref.gradients64(up, up_bias, down, down_bias, x, K)
    assert abs(loss64 - want_loss) <= 1e-13 * abs(want_loss)
    assert np.abs(g64["up_bias"] - want["up_bias"]).max() <= 1e-12 * np.abs(want["up_bias"]).max()
    model = ref.Model(up, down, up_bias, down_bias, K)
    loss, g, (rows, fs) = ref.gradients(model, x)
    kept = np.zeros_like(mask)
    kept[rows, fs] = True
    assert np.array_equal(kept, mask), "float32 and float64 keep different features for this draw"
    _, bounds = ref.gradient_bounds(up, up_bias, down, down_bias, x, K)
    assert (np.abs(g["up_bias"].astype(np.float64) - want["up_bias"]) <= bounds["up_bias"]).all()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_against_float64_and_torch(wd):
    rng = np.random.default_rng(11)
    n, lr, betas, eps = 4000, 3e-4, (0.9, 0.999), 1e-8
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32) for _ in range(3)]
    grads[1][::7] = 0.0                                   # momentum without a gradient
    # torch.optim.AdamW in float64 is the float64 formula
    tp = torch.tensor(p0.astype(np.float64), requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    p32, m32, v32 = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, g in enumerate(grads, start=1):
        tp.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        p64, m64, v64 = ref.adamw64(p64, m64, v64, g, t, lr, betas, eps, wd)
        assert np.allclose(tp.detach().numpy(), p64, rtol=1e-13, atol=0)
        # one f32 step from the f32 state against one float64 step from the same state, on the same gradient
        q64, _, _ = ref.adamw64(p32, m32, v32, g, t, lr, betas, eps, wd)
        before = p32
        p32, m32, v32 = ref.adamw32(p32, m32, v32, g, t, lr, betas, eps, wd)
        d32, d64 = p32.astype(np.float64) - before, q64 - before
        # without decay: codec training's bound, the ten-odd roundings of the quotient under 1e-5 of the step and one
        # ulp for the subtraction.  With decay two more things happen at p's magnitude: the constant (float)(1 - lr wd) is off by at
        # most 2^-24 of itself, which moves p * decay by less than ulp(p), and the product rounds once (half an ulp; the subtraction's
        # half makes the first ulp whole): 2 ulp(p)
        ulps = 1 if wd == 0.0 else 2
        assert (np.abs(d32 - d64) <= 1e-5 * np.abs(d64) + ulps * np.spacing(np.abs(before))).all(), t


def test_ties_at_the_threshold_get_no_gradient():
    up, x, K, want_counts = sae_ref.tie_case()
    H, E = up.shape
    rng = np.random.default_rng(2)
    down = rng.integers(-2, 3, (E, H)).astype(np.float32)
    down_bias = rng.integers(-2, 3, E).astype(np.float32)
    model = ref.Model(up, down, None, down_bias, K)
    loss, g, (rows, fs) = ref.gradients(model, x)
    assert np.array_equal(np.bincount(rows, minlength=x.shape[0]), want_counts)
    assert not (rows == 0).any() and not (rows == 7).any()       # row 0: top_k + 1 equal values; row 7: all zero
    z = sae_ref.pre_activations(up, x)
    for i, f in zip(rows, fs):
        a = np.maximum(z[i], 0)
        assert a[f] > np.sort(a)[H - K - 1]                       # strictly above the threshold
    want_loss, want = torch_gradients(up, None, down, down_bias, x, K)
    assert np.isclose(loss, want_loss, rtol=1e-6)
    assert np.allclose(g["up"], want["up"], rtol=1e-5, atol=1e-6) and np.allclose(g["down_t"].T, want["down"], rtol=1e-5, atol=1e-6)
    never = np.setdiff1d(np.arange(H), fs)
    assert not g["up"][never].any() and not g["down_t"][never].any() and not want["up"][never].any()


def test_a_nan_row_refuses_the_step():
    up, down, down_bias, x = case(SHAPES[0], 0)
    model = ref.Model(up, down, None, down_bias, 16)
    bad = x.copy()
    bad[5, 2] = np.nan
    before = {k: v.copy() for k, v in model.params().items()}
    assert ref.step(model, bad) is None and model.t == 0 and not model.counters.any()
    assert all(np.array_equal(before[k], v) for k, v in model.params().items())
    assert ref.step(model, x) is not None and model.t == 1 and model.counters.sum() > 0
