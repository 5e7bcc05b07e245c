"""CPU checks of tests/sae_ref.py, the restatement tests/test_gpu_sae.py holds the device to: its selection is torch.kthvalue plus the
strict mask of the reference's sae/model.py:32-41, its hand-made tie cases have the counts their comments claim, its squared-error order
is a sum, and a checkpoint's state dict maps onto the constructor's tensors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sae_ref as ref


def torch_selection(a, top_k):
    """model.py:32-41 from the relu on, written anew: threshold by kthvalue, strict mask."""
    x = F.relu(torch.from_numpy(np.asarray(a, np.float32)))
    thresholds = torch.kthvalue(x, k=x.shape[-1] - top_k, dim=-1).values.unsqueeze(-1).expand_as(x)
    mask = x > thresholds
    return mask.numpy(), torch.where(mask, x, torch.zeros_like(x)).numpy()


def dense_of(counts, feats, acts, d_hidden):
    mask = np.zeros((counts.size, d_hidden), bool)
    vals = np.zeros((counts.size, d_hidden), np.float32)
    for b in range(counts.size):
        f = feats[b, :counts[b]].astype(np.int64)
        mask[b, f] = True
        vals[b, f] = acts[b, :counts[b]]
    return mask, vals


def activation_sets():
    rng = np.random.default_rng(5)
    yield "normals", rng.standard_normal((9, 300)).astype(np.float32)
    yield "tie-heavy integers", rng.integers(-3, 4, (40, 64)).astype(np.float32)
    yield "two values", rng.integers(0, 2, (40, 33)).astype(np.float32)
    z = rng.integers(-2, 3, (6, 50)).astype(np.float32)
    z[1] = 0
    z[3] = -1
    z[4] = 7
    yield "all-zero, all-negative and all-equal rows", z
    yield "with infinities", np.where(rng.random((8, 40)) < 0.1, np.float32(np.inf), rng.standard_normal((8, 40)).astype(np.float32))


@pytest.mark.parametrize("name,z", list(activation_sets()))
def test_selection_is_kthvalue_and_the_strict_mask(name, z):
    d_hidden = z.shape[1]
    for top_k in sorted({1, 2, d_hidden // 3, d_hidden - 2, d_hidden - 1}):
        counts, feats, acts = ref.select(z, top_k)
        mask, vals = dense_of(counts, feats, acts, d_hidden)
        want_mask, want_vals = torch_selection(z, top_k)
        assert np.array_equal(mask, want_mask) and np.array_equal(vals.view(np.uint32), want_vals.view(np.uint32)), (name, top_k)
        assert counts.max() <= top_k
        for b in range(z.shape[0]):                       # canonical order, padding
            a, f = acts[b, :counts[b]], feats[b, :counts[b]].astype(np.int64)
            assert all((a[i] > a[i + 1]) or (a[i] == a[i + 1] and f[i] < f[i + 1]) for i in range(len(a) - 1))
            assert (feats[b, counts[b]:] == ref.NONE).all() and not acts[b, counts[b]:].view(np.uint32).any()


def test_nan_rows_are_invalid():
    z = np.random.default_rng(6).standard_normal((3, 20)).astype(np.float32)
    z[1, 7] = np.nan
    counts, feats, acts = ref.select(z, 4)
    assert counts[1] == ref.NONE and (feats[1] == ref.NONE).all() and not acts[1].any()
    assert counts[0] == 4 and counts[2] == 4
    assert ref.counters(counts, feats, 20).sum() == 8


def test_tie_cases_have_the_counts_their_comments_claim():
    up, x, top_k, want = ref.tie_case()
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    z = ref.pre_activations(up, x)
    assert np.array_equal(z, x @ up.T)                    # small integers: every order of summation is exact
    assert not np.signbit(z[3][up[:, 3] == 0]).any()      # -0.0 products leave the chain's +0 as it is
    counts, feats, acts = ref.select(z, top_k)
    assert np.array_equal(counts, want), counts
    mask, _ = dense_of(counts, feats, acts, up.shape[0])
    assert np.array_equal(mask, torch_selection(z, top_k)[0])


def test_reconstruction_and_error_against_float64():
    rng = np.random.default_rng(7)
    d_emb, d_hidden, top_k, rows = 300, 90, 12, 5         # 300: two steps of the 256 lanes, the second ragged
    up = rng.standard_normal((d_hidden, d_emb)).astype(np.float32) / 16
    down = rng.standard_normal((d_emb, d_hidden)).astype(np.float32) / 8
    bias = rng.standard_normal(d_emb).astype(np.float32)
    x = rng.standard_normal((rows, d_emb)).astype(np.float16).astype(np.float32)
    counts, feats, acts = ref.encode(up, x, top_k)
    r = ref.reconstruct(down, bias, counts, feats, acts)
    mask, vals = dense_of(counts, feats, acts, d_hidden)
    want = vals.astype(np.float64) @ down.astype(np.float64).T + bias
    assert np.allclose(r, want, rtol=1e-5, atol=1e-5)
    s = ref.sq_errors(r, x)
    assert np.allclose(s, ((r - x).astype(np.float32).astype(np.float64) ** 2).sum(axis=1), rtol=1e-12)
    assert np.array_equal(ref.counters(counts, feats, d_hidden), np.bincount(np.nonzero(mask)[1], minlength=d_hidden))


def test_state_dict_maps_onto_the_constructor(mse):
    """up_proj / down_proj as model.py:20-22 builds them: two Linears, the second's weight the transpose of the first's."""
    d_emb, d_hidden = 12, 40
    for up_bias in (False, True):
        up_proj = torch.nn.Linear(d_emb, d_hidden, bias=up_bias)
        down_proj = torch.nn.Linear(d_hidden, d_emb)
        down_proj.weight = torch.nn.Parameter(up_proj.weight.T.clone())
        sd = {"up_proj.weight": up_proj.weight, "down_proj.weight": down_proj.weight, "down_proj.bias": down_proj.bias}
        if up_bias:
            sd["up_proj.bias"] = up_proj.bias
        up, down, ub, db = mse.SparseAutoencoder.state_dict_tensors(sd)
        assert up.shape == (d_hidden, d_emb) and down.shape == (d_emb, d_hidden) and db.shape == (d_emb,)
        assert up.dtype == down.dtype == db.dtype == np.float32
        assert np.array_equal(up, up_proj.weight.detach().numpy()) and np.array_equal(down, up.T)
        assert np.array_equal(db, down_proj.bias.detach().numpy())
        assert (ub is None) == (not up_bias) and (ub is None or np.array_equal(ub, up_proj.bias.detach().numpy()))
