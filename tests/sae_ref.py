"""numpy restatement of csrc/sae.hip: the sparse-autoencoder encode of the reference's sae/model.py:31-43 in the device's own arithmetic.
tests/test_sae_host.py holds it to torch.kthvalue on the CPU; tests/test_gpu_sae.py holds the device to it, bit for bit.

The rule, as the header of csrc/sae.hip states it:
  pre-activation  z[b][j] = fma(up[j][K-1], x[b][K-1], ... fma(up[j][0], x[b][0], +0)): one f32 fma chain, k ascending (describe_ref's);
                  with a bias, z += up_bias[j], one f32 add
  relu            a = z where z > 0, else +0
  threshold       t = the (top_k + 1)-th largest a (torch.kthvalue(a, d_hidden - top_k)); kept = { j : a_j > t }
  order           activation descending, then feature ascending; unused slots: feature 0xFFFFFFFF, activation +0
  NaN             a row with a NaN pre-activation is invalid: count 0xFFFFFFFF, no features, nothing counted
  reconstruction  r_d = fma(a, down[d][f], r_d) over the kept features in that order, from down_bias[d] (or +0)
  squared error   e_d = f32(r_d - x_d); S_t = sum of f64(e_d)^2 over d = t, t + 256, ... ascending from +0 (t < 256); then the tree
                  S_t += S_{t + o}, o = 128, 64, ..., 1; the row's error is S_0.  NaN for an invalid row
Nothing in it names the row's place in the call, the number of rows, the grid or how d_hidden is split."""
import numpy as np

from describe_ref import fma32, pre_activations as _chain

NONE = 0xFFFFFFFF
SUM_LANES = 256


def pre_activations(up, x, up_bias=None):
    """[rows, d_hidden] f32"""
    with np.errstate(invalid="ignore", over="ignore"):
        z = _chain(up, x)
        if up_bias is not None:
            z = (z + np.asarray(up_bias, np.float32)[None, :]).astype(np.float32)
    return z


def relu(z):
    z = np.asarray(z, np.float32)
    return np.where(z > 0, z, np.float32(0.0)).astype(np.float32)


def select(z, top_k):
    """(counts u32 [rows], features u32 [rows, top_k], activations f32 [rows, top_k]) from the pre-activations, by a full sort."""
    z = np.asarray(z, np.float32)
    rows, d_hidden = z.shape
    assert 1 <= top_k < d_hidden
    counts = np.zeros(rows, np.uint32)
    feats = np.full((rows, top_k), NONE, np.uint32)
    acts = np.zeros((rows, top_k), np.float32)
    for b in range(rows):
        if np.isnan(z[b]).any():
            counts[b] = NONE
            continue
        a = relu(z[b])
        order = np.argsort(-a, kind="stable")          # activation descending, feature ascending among equals
        t = a[order[top_k]]                            # the (top_k + 1)-th largest
        kept = order[a[order] > t]
        counts[b] = kept.size
        feats[b, :kept.size] = kept
        acts[b, :kept.size] = a[kept]
    return counts, feats, acts


def encode(up, x, top_k, up_bias=None):
    return select(pre_activations(up, x, up_bias), top_k)


def reconstruct(down, down_bias, counts, feats, acts):
    """f32 [rows, d_emb]; down [d_emb, d_hidden] as the checkpoint stores it"""
    down_t = np.ascontiguousarray(np.asarray(down, np.float32).T)
    rows, d_emb = counts.size, down_t.shape[1]
    r = np.zeros((rows, d_emb), np.float32)
    if down_bias is not None:
        r += np.asarray(down_bias, np.float32)[None, :]
    valid = counts != NONE
    c = np.where(valid, counts, 0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(int(c.max()) if rows else 0):
            on = np.nonzero(c > i)[0]
            r[on] = fma32(acts[on, i][:, None], down_t[feats[on, i].astype(np.int64)], r[on])
    r[~valid] = np.nan
    return r


def sq_errors(recon, x):
    """f64 [rows] in the stated order; x: the f32 widening of the f16 rows"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = (np.asarray(recon, np.float32) - np.asarray(x, np.float32)).astype(np.float32).astype(np.float64)
        sq = e * e
        rows, d = sq.shape
        steps = -(-d // SUM_LANES)
        pad = np.zeros((rows, steps * SUM_LANES), np.float64)      # a lane past d adds nothing
        pad[:, :d] = sq
        pad = pad.reshape(rows, steps, SUM_LANES)
        s = np.zeros((rows, SUM_LANES), np.float64)
        for j in range(steps):
            lanes = min(SUM_LANES, d - j * SUM_LANES)
            s[:, :lanes] = s[:, :lanes] + pad[:, j, :lanes]
        o = SUM_LANES // 2
        while o:
            s[:, :o] = s[:, :o] + s[:, o:2 * o]
            o //= 2
    return s[:, 0].copy()


def counters(counts, feats, d_hidden):
    """u64 [d_hidden]: how many valid rows keep each feature"""
    kept = [feats[b, :counts[b]] for b in range(counts.size) if counts[b] != NONE]
    flat = np.concatenate(kept).astype(np.int64) if kept else np.zeros(0, np.int64)
    return np.bincount(flat, minlength=d_hidden).astype(np.uint64)


# ---- hand-made tie cases ------------------------------------------------------------------------------------------------------------
TIE_D_EMB, TIE_D_HIDDEN, TIE_TOP_K = 8, 300, 16


def tie_case():
    """(up [300, 8], x [8, 8] f32 exactly representable in f16, top_k, expected counts).  Row r of x is the unit vector e_r (row 3:
    -e_3), so its pre-activations are column r of up: small integers, set by hand.  There is no bias."""
    H, K = TIE_D_HIDDEN, TIE_TOP_K
    rng = np.random.default_rng(41)
    up = np.zeros((H, TIE_D_EMB), np.float32)
    x = np.eye(TIE_D_EMB, dtype=np.float32)
    want = np.zeros(TIE_D_EMB, np.uint32)
    # row 0: the top_k + 1 largest are all 5, the rest 1 .. 4: t = 5 and nothing is above it -> 0
    col = rng.integers(1, 5, H).astype(np.float32)
    col[rng.permutation(H)[:K + 1]] = 5
    up[:, 0], want[0] = col, 0
    # row 1: three positives (fewer than top_k + 1), the rest negative or zero: t = 0 -> all 3
    col = -rng.integers(0, 4, H).astype(np.float32)
    col[[7, 130, 299]] = [2, 9, 2]
    up[:, 1], want[1] = col, 3
    # row 2: all negative -> 0
    up[:, 2], want[2] = -rng.integers(1, 6, H).astype(np.float32), 0
    # row 3: x = -e_3: zero weights give -0.0 products, which never count as positive; the five weights -3 give +3 -> 5
    col = np.zeros(H, np.float32)
    col[[0, 127, 128, 255, 256]] = -3
    up[:, 3], want[3] = col, 5
    x[3, 3] = -1
    # row 4: 300 distinct values: exactly top_k above the (top_k + 1)-th -> 16
    up[:, 4], want[4] = rng.permutation(H).astype(np.float32) + 1, K
    # row 5: top_k - 1 distinct values above 7, then four sevens: the (top_k + 1)-th largest is 7 -> top_k - 1 = 15
    col = rng.integers(1, 7, H).astype(np.float32)
    pos = rng.permutation(H)
    col[pos[:K - 1]] = np.arange(K - 1) + 8
    col[pos[K - 1:K + 3]] = 7
    up[:, 5], want[5] = col, K - 1
    # row 6: exactly top_k + 1 positives, all different: t = the smallest of them -> 16
    col = np.zeros(H, np.float32)
    col[rng.permutation(H)[:K + 1]] = np.arange(K + 1) + 1
    up[:, 6], want[6] = col, K
    # row 7: all zero -> 0
    want[7] = 0
    return up, x, K, want
