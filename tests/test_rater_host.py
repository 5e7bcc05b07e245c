"""CPU checks of tests/rater_ref.py, the restatement tests/test_gpu_rater.py holds the device to: its exponential is within EXP_ULPS of
float64, its loss and gradients are those of the reference's module (meme-rater/model.py:18-52 under F.binary_cross_entropy,
train.py:63-68) written anew in float64 torch, its update is sae_train_ref's AdamW, its variance is torch.var's, and the exported wide
model scores the member mean."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import describe_ref
import rater_ref as ref
import sae_train_ref

SHAPES = [(8, 3, 3, 4), (33, 2, 1, 5)]   # (E, M, C, B)


# ---- exp_fixed ----------------------------------------------------------------------------------------------------------------------------
def exp_sweep_chunks(per_binade=227000, seed=0):
    """f32 inputs, a chunk at a time: both signs of every binade from 2^-30 up to the clamp at 87 (the last one cut there), per_binade
    random mantissas each (74 x 227000 > 2^24 inputs), then both clamp ends, values past them, and the two f32 neighbours of every
    multiple of ln2 / 2 in range with the multiple itself"""
    rng = np.random.default_rng(seed)
    for e in range(-30, 7):
        lo, hi = 2.0 ** e, min(2.0 ** (e + 1), 87.0)
        mag = rng.uniform(lo, hi, per_binade).astype(np.float32)
        yield mag
        yield -mag
    k = np.arange(-251, 252)
    mid = (k * (np.log(2.0) / 2)).astype(np.float32)
    yield np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)),
                          np.array([-87.0, 87.0, -87.5, 88.0, -100.0, 100.0, -np.inf, np.inf, 0.0, -0.0], np.float32)])


def exp_ulps(x):
    """|exp_fixed(x) - exp(clamped x)| in ulps of the f32 nearest the true value"""
    got = ref.exp_fixed(x).astype(np.float64)
    true = np.exp(np.clip(x.astype(np.float64), -87.0, 87.0))
    return np.abs(got - true) / np.spacing(true.astype(np.float32)).astype(np.float64)


def test_exp_fixed_stays_within_exp_ulps_of_float64():
    worst, count = 0.0, 0
    for x in exp_sweep_chunks():
        worst = max(worst, float(exp_ulps(x).max()))
        count += x.size
    print("exp_fixed: largest error %.4f ulp over %d inputs" % (worst, count))
    assert count >= 1 << 24
    assert worst <= ref.EXP_ULPS
    assert ref.EXP_ULPS == int(np.ceil(worst))              # the constant is the measured maximum rounded up, no more


def test_exp_fixed_edges():
    x = np.array([-87.0, 87.0, -1000.0, 1000.0, -np.inf, np.inf, 0.0], np.float32)
    got = ref.exp_fixed(x)
    assert np.array_equal(got[2:6], got[[0, 1, 0, 1]]) and got[6] == 1.0
    assert np.isnan(ref.exp_fixed(np.array([np.nan], np.float32)))[0]
    # sig never leaves the normal numbers: the smallest is 1 / (1 + e^87)
    s = ref.sig(np.array([-1000.0, -87.0, 0.0, 87.0, 1000.0], np.float32))
    assert s[0] == s[1] and s[1] >= np.finfo(np.float32).tiny and s[2] == 0.5 and s[3] == 1.0 and s[4] == 1.0


# ---- the restatement against torch ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(shape, seed):
    E, M, C, B = shape
    rng = np.random.default_rng(100 * seed + E)
    up, bias, down = ref.random_weights(E, M, C, rng)
    down = (down * 4).astype(np.float32)                     # scores of order 1: the head is off its linear part, |z| stays below 8
    x = rng.standard_normal((M, 2 * B, E)).astype(np.float16).astype(np.float32)
    y = rng.choice([0.1, 0.3, 0.5, 0.7, 0.9], (M, B, C)).astype(np.float32)
    return up, bias, down, x, y


class TorchMember(nn.Module):
    """model.py:18-29 with n_hidden = 1 and no dropout"""

    def __init__(self, E, C):
        super().__init__()
        self.hidden = nn.Linear(E, E, dtype=torch.float64)
        self.output = nn.Linear(E, C, dtype=torch.float64)

    def forward(self, x):
        return self.output(F.silu(self.hidden(x)))


def torch_gradients(up, bias, down, M, x, y, dtype=torch.float64):
    """model.py:31-52 and train.py:66-68: the members, sigmoid(s1 - s2), F.binary_cross_entropy, backward; an output bias of 0.25 is
    carried along to show that it does not matter -> (loss, grads in the wide layout, the output biases' gradients)"""
    E, C = up.shape[1], down.shape[0]
    members = [TorchMember(E, C).to(dtype) for _ in range(M)]
    with torch.no_grad():
        for m, mod in enumerate(members):
            mod.hidden.weight.copy_(torch.tensor(up[m * E:(m + 1) * E]).to(dtype))
            mod.hidden.bias.copy_(torch.tensor(bias[m * E:(m + 1) * E]).to(dtype))
            mod.output.weight.copy_(torch.tensor(down[:, m * E:(m + 1) * E]).to(dtype))
            mod.output.bias.fill_(0.25)
    xb, yb = torch.tensor(x).to(dtype), torch.tensor(y).to(dtype)
    with torch.enable_grad():                                  # other tests of the suite switch autograd off for the process
        s1 = torch.stack([mod(xb[m, 0::2]) for m, mod in enumerate(members)])
        s2 = torch.stack([mod(xb[m, 1::2]) for m, mod in enumerate(members)])
        loss = F.binary_cross_entropy(torch.sigmoid(s1 - s2), yb)
        loss.backward()
    g = {"up": np.concatenate([mod.hidden.weight.grad.numpy() for mod in members]),
         "bias": np.concatenate([mod.hidden.bias.grad.numpy() for mod in members]),
         "down": np.concatenate([mod.output.weight.grad.numpy() for mod in members], axis=1)}
    return float(loss.detach()), g, np.stack([mod.output.bias.grad.numpy() for mod in members])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_loss_and_gradients_against_float64_torch(shape, seed):
    E, M, C, B = shape
    up, bias, down, x, y = case(shape, seed)
    loss64, g64, z = ref.gradients64(up, bias, down, M, x, y)
    assert np.abs(z).max() < 8 and np.abs(z).max() > 0.5     # in float64 first: off the linear part, far from saturation
    want_loss, want, out_bias_grad = torch_gradients(up, bias, down, M, x, y)
    assert np.abs(out_bias_grad).max() <= 1e-17              # g - g: the output bias has no gradient
    assert abs(loss64 - want_loss) <= 1e-13 * abs(want_loss)
    for name in want:
        assert np.abs(g64[name] - want[name]).max() <= 1e-12 * np.abs(want[name]).max(), name
    model = ref.Model(up, bias, down, M)
    loss, g, _ = ref.gradients(model, x, y)
    d_loss, bounds, _ = ref.gradient_bounds(up, bias, down, M, x, y)
    assert abs(loss - want_loss) <= d_loss
    worst = {"loss": abs(loss - want_loss) / d_loss}
    for name in want:
        err = np.abs(g[name].astype(np.float64) - want[name])
        assert (err <= bounds[name]).all(), name
        worst[name] = float((err / bounds[name]).max())
    print("rater gradients %s seed %d: largest error / bound %s" % (shape, seed, {k: "%.3g" % v for k, v in worst.items()}))


def test_saturated_head_keeps_its_gradient_where_torch_drops_it():
    """|z| > 20: p rounds to 1 in f32.  torch's clamped log and its p (1 - p) factor give a zero gradient; the rule keeps (p - y) / N"""
    E, M, C, B = 8, 1, 1, 1
    rng = np.random.default_rng(4)
    up, bias, down = ref.random_weights(E, M, C, rng)
    x = np.zeros((M, 2, E), np.float32)
    x[0, 0], x[0, 1] = 4.0, -4.0
    down = (np.sign(up.sum(axis=1))[None, :] * 8).astype(np.float32)   # every unit that the first row switches on pushes its score up
    y = np.full((M, B, C), 0.1, np.float32)
    model = ref.Model(up, bias, down, M)
    loss, g, s = ref.gradients(model, x, y)
    z = float(s[0, 0, 0] - s[0, 1, 0])
    assert z > 20 and ref.sig(np.float32(z)) == 1.0
    _, t32, _ = torch_gradients(up, bias, down, M, x, y, dtype=torch.float32)
    assert not any(a.any() for a in t32.values())             # torch, in float32: nothing moves
    want_g = (np.float32(1.0) - np.float32(0.1)) * np.float32(1.0)      # (p - y) / N with N = 1
    u, h = ref.hidden(model, x)
    assert np.array_equal(g["down"][0], describe_ref.fma32(-want_g, h[0, 1], (want_g * h[0, 0]).astype(np.float32)))
    assert g["down"].any() and g["up"].any() and g["bias"].any()
    assert np.isclose(loss, 0.9 * 100.0, rtol=1e-6)           # log(1 - p) clamped at -100, as torch clamps it


def test_a_non_finite_row_refuses_the_step():
    up, bias, down, x, y = case(SHAPES[0], 0)
    for bad_value in (np.nan, np.inf):
        model = ref.Model(up, bias, down, SHAPES[0][1])
        bad = x.copy()
        bad[1, 3, 2] = bad_value
        assert ref.step(model, bad, y) is None and model.t == 0
        assert all(np.array_equal(a, b) for a, b in zip((up, bias, down), (model.up, model.bias, model.down)))
        assert ref.step(model, x, y) is not None and model.t == 1


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_step_is_sae_train_refs_adamw_on_the_restated_gradients(wd):
    E, M, C, B = SHAPES[1]
    up, bias, down, x, y = case(SHAPES[1], 0)
    model = ref.Model(up, bias, down, M, weight_decay=wd)
    for t in (1, 2, 3):
        before = {k: v.copy() for k, v in model.params().items()}
        m0, v0 = {k: v.copy() for k, v in model.m.items()}, {k: v.copy() for k, v in model.v.items()}
        _, g, _ = ref.gradients(model, x, y)
        assert ref.step(model, x, y) is not None and model.t == t
        for name in before:
            p32, m32, v32 = sae_train_ref.adamw32(before[name], m0[name], v0[name], g[name], t, model.lr, model.betas, model.eps, wd)
            assert np.array_equal(p32, model.params()[name]) and np.array_equal(m32, model.m[name]) and np.array_equal(v32, model.v[name])
            q64, _, _ = sae_train_ref.adamw64(before[name], m0[name], v0[name], g[name], t, model.lr, model.betas, model.eps, wd)
            d32, d64 = model.params()[name].astype(np.float64) - before[name], q64 - before[name]
            ulps = 1 if wd == 0.0 else 2                       # test_sae_train_host.py's bound, derived there
            assert (np.abs(d32 - d64) <= 1e-5 * np.abs(d64) + ulps * np.spacing(np.abs(before[name]))).all(), (name, t)
            if t == 1:                                         # the first step's moment is (1 - beta1) g: it pins every gradient bit
                assert np.array_equal(model.m[name], ((np.float32(1) - np.float32(0.9)) * g[name]).astype(np.float32))


# ---- variance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 16])
def test_pair_variance_against_float64_torch(M):
    """Per channel, with u = 2^-24 and e = EXP_ULPS: every p_m is off by at most dp = (2 e + 4) u (sig's roundings and the subtraction of
    the scores, |sig'| <= 1/4, p <= 1); the mean by dp + gamma_M (a sum of M terms and a divide; mean <= 1); each deviation d by
    dd = 2 dp + gamma_M + u; the sum of squares by sum_m (2 |d| dd + dd^2) + gamma_(M + 1) sum_m d^2, the divide by M - 1 adds u."""
    rng = np.random.default_rng(20 + M)
    n, C = 64, 3
    table = rng.standard_normal((n, M, C)).astype(np.float32)
    a, b = rng.integers(0, n, 200), rng.integers(0, n, 200)
    a[:4] = b[:4]                                              # a row against itself
    got = ref.pair_variance(table, a, b)
    assert not got[:4].any() and not np.signbit(got[:4]).any()      # every p is 1/2: variance +0
    z = torch.tensor(table.astype(np.float64))
    p = torch.sigmoid(z[a] - z[b]).permute(1, 0, 2)            # [M, pairs, C]
    want = torch.var(p, dim=0).max(-1).values.numpy()
    u, g = ref.U, ref.gamma
    dp = (2 * ref.EXP_ULPS + 4) * u
    dd = 2 * dp + g(M) + u
    d = (p - p.mean(dim=0)).abs().numpy()
    bound = ((2 * d * dd + dd * dd).sum(axis=0) + g(M + 1) * (d * d).sum(axis=0)) / (M - 1)
    bound = (bound + u * (torch.var(p, dim=0).numpy() + bound)).max(axis=-1)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all()
    print("pair variance M = %d: largest error / bound %.3g" % (M, float((err[4:] / bound[4:]).max())))


def test_top_pairs_orders_ties_by_pair_index():
    v = np.array([0.25, 0.5, 0.25, 0.0, 0.5, 0.25], np.float32)
    assert ref.top_pairs(v, 6).tolist() == [1, 4, 0, 2, 5, 3]
    assert ref.top_pairs(v, 3).tolist() == [1, 4, 0]
    # the product's host-side ordering is the same rule
    order = np.lexsort((np.arange(v.size), -v.astype(np.float64)))
    assert order.tolist() == [1, 4, 0, 2, 5, 3]


def test_map_rating_is_the_references_table():
    assert ref.map_rating("1,2+,eq").tolist() == [0.9, 0.3, 0.5] and ref.map_rating("2,1p,2p,1+").tolist() == [0.1, 0.7, 0.3, 0.7]
    with pytest.raises(KeyError):
        ref.map_rating("3")


# ---- export ------------------------------------------------------------------------------------------------------------------------------
def test_exported_wide_model_scores_the_member_mean():
    """ensemble_to_wide_model.py:59-68: the wide model under score_model.rs's d_emb / d_hidden = 1 / M scale is the mean of the members"""
    E, M, C = 33, 3, 2
    rng = np.random.default_rng(9)
    up, bias, down = ref.random_weights(E, M, C, rng)
    x = rng.standard_normal((20, E)).astype(np.float16).astype(np.float32)
    s = ref.member_scores(ref.Model(up, bias, down, M), x)
    want = s.astype(np.float64).mean(axis=1)
    got = describe_ref.score_rows(up, bias, down, x)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_planted_utility_is_learned_by_the_restatement_alone():
    before, after, _ = ref.planted_run()
    print("planted utility, 256 held-out pairs: loss %.4f -> %.4f, correctly ordered %.3f -> %.3f" % (before[0], after[0], before[1], after[1]))
    assert after[0] < before[0] - 0.05 and after[1] > before[1] + 0.2 and after[1] > 0.8
