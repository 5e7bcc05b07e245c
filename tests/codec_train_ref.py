"""Restatement of the codec trainer (include/mse.h mse_pq_trainer) in numpy and oracle/orc.py's PQ -- test
infrastructure shared by tests/test_codec_train_host.py and tests/test_gpu_codec_train.py, like tests/grouped_ref.py.

Bit-exact pieces: the order-free sum, its exponent, the k-means step, the rotated second moment (all through the oracle's rotation
and assignment).  Float64 pieces with derived error bounds: the residual product, the loss, the gradient, the Adam step, the cross
matrix.  `train_f64` is the whole algorithm in float64, to check on the CPU what the end-to-end test asks of the device."""
import numpy as np

U32 = 2.0 ** -24      # unit roundoff of f32
U64 = 2.0 ** -53


def ceil_log2(n):
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return lg


def fixed_exponent(vmax, n):
    """E = 61 - ceil(log2 n) - ex with vmax = f 2^ex, f in [0.5, 1); ex = 0 at vmax = 0."""
    vmax = float(np.float32(vmax))
    ex = int(np.frexp(vmax)[1]) if vmax != 0.0 else 0
    return 61 - ceil_log2(int(n)) - ex


def accumulate_by_code(v, code, n_cells):
    """The order-free sum: -> (sums [n_cells, w] int64, E)."""
    v = np.asarray(v, np.float32)
    v = v.reshape(v.shape[0], -1)
    if not np.isfinite(v).all():
        raise ValueError("non-finite input")
    E = fixed_exponent(np.abs(v).max() if v.size else 0.0, v.shape[0])
    terms = np.rint(np.ldexp(v.astype(np.float64), E)).astype(np.int64)     # exact scaling, round-half-even
    sums = np.zeros((n_cells, v.shape[1]), np.int64)
    np.add.at(sums, np.asarray(code, np.int64), terms)
    return sums, E


def sums_with_exponent(v, code, n_cells, E):
    terms = np.rint(np.ldexp(np.asarray(v, np.float32).astype(np.float64), E)).astype(np.int64)
    sums = np.zeros((n_cells, terms.shape[1]), np.int64)
    np.add.at(sums, np.asarray(code, np.int64), terms)
    return sums


def rotate(orc, T, x):
    d = T.shape[0]
    return orc.PQ(np.zeros((1, d), np.float32), T, d, d).apply_transform(x)


def assign(orc, xr, cent, dpc):
    d = xr.shape[1]
    return orc.PQ(cent, np.eye(d, dtype=np.float32), dpc, d).quantize_batch(xr, pre_transformed=True)


def quantized(codes, cent, dpc):
    """Y [n, d]: the concatenation of the assigned centroids."""
    n, nch = codes.shape
    y = np.empty((n, nch * dpc), np.float32)
    for s in range(nch):
        y[:, s * dpc:(s + 1) * dpc] = cent[codes[:, s], s * dpc:(s + 1) * dpc]
    return y


def kmeans_step(orc, xr, cent, dpc):
    """One k-means step as defined: -> (new centroids, codes, empty cells)."""
    n, d = xr.shape
    n_cells = cent.shape[0]
    codes = assign(orc, xr, cent, dpc)
    E = fixed_exponent(np.abs(xr).max(), n)
    out = cent.copy()
    empty = 0
    for s in range(d // dpc):
        S = sums_with_exponent(xr[:, s * dpc:(s + 1) * dpc], codes[:, s], n_cells, E)
        cnt = np.bincount(codes[:, s], minlength=n_cells)
        has = cnt > 0
        empty += int((~has).sum())
        mean = (S[has].astype(np.float64) / cnt[has].astype(np.float64)[:, None]) * 2.0 ** -E
        out[has, s * dpc:(s + 1) * dpc] = mean.astype(np.float32)
    return out, codes, empty


def rotated_moment(orc, T, C0):
    """C = T C0 T^T the way the trainer forms it: rows of C0 rotated, transposed, rows rotated again (bit-exact)."""
    w = rotate(orc, T, C0)
    return rotate(orc, T, np.ascontiguousarray(w.T))


def residual_product_f64(xr, codes, cent, Cm, dpc):
    """-> (R f32, G f64, bound on |G_device - G|, l_row f64, bound on |l_row_device - l_row|).
    G: an f32 fma chain of length K = d has |error| <= gamma_K sum_k |r_k C_kj| ~ K u sum_k |r_k| |C_kj|.
    l_row = sum_j r_j G_j in f32, any order: the G error weighted by |r_j|, plus d u sum_j |r_j| |G_j| for the d products and adds."""
    R = xr - quantized(codes, cent, dpc)          # f32 subtraction
    R64, C64 = R.astype(np.float64), Cm.astype(np.float64)
    G = R64 @ C64
    K = xr.shape[1]
    bG = K * U32 * (np.abs(R64) @ np.abs(C64))
    l = (R64 * G).sum(axis=1)
    bl = 1.001 * ((np.abs(R64) * bG).sum(axis=1) + K * U32 * (np.abs(R64) * (np.abs(G) + bG)).sum(axis=1))
    return R, G, bG, l, bl


def loss_and_gradient_f64(xr, codes, cent, Cm, dpc):
    """-> (L, bound on |L_device - L|, grad [n_cells, d] f64, bound on |grad_device - grad|).
    The fixed-point step adds at most half a unit, 2^-(E+1) <= 2^(ceil(log2 n) - 61) vmax, per term: n terms, against sums of order vmax;
    the conversions and the final rounding to f32 add u |grad|.  The factor 1.01 covers the second-order terms."""
    n, d = xr.shape
    n_cells = cent.shape[0]
    R, G, bG, l, bl = residual_product_f64(xr, codes, cent, Cm, dpc)
    fix = 2.0 ** (ceil_log2(n) - 60)
    L = l.sum() / n
    bL = 1.01 * (bl.sum() / n + fix * (np.abs(l) + bl).max() + 8 * U64 * np.abs(l).sum() / n)
    grad = np.zeros((n_cells, d), np.float64)
    bg = np.zeros((n_cells, d), np.float64)
    gmax = (np.abs(G) + bG).max()
    for s in range(d // dpc):
        sl = slice(s * dpc, (s + 1) * dpc)
        np.add.at(grad[:, sl], codes[:, s], G[:, sl])
        np.add.at(bg[:, sl], codes[:, s], bG[:, sl] + fix * gmax)
    grad *= -2.0 / n
    bg = 1.01 * (bg * 2.0 / n + 2 * U32 * np.abs(grad))
    return L, bL, grad, bg


def adam_step_f64(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's step number t + 1 in float64: -> (p, m, v)."""
    t = t + 1
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps)
    return p, m, v


def cross_f64(xr, y, n_cells, E):
    """-> (M = X'^T Y in float64, bound on |M_device - M|).  The device sums X' per cell in fixed point (half a unit 2^-(E+1) per
    row, each weighted by a centroid entry) and multiplies out in float64."""
    x64, y64 = xr.astype(np.float64), y.astype(np.float64)
    n = xr.shape[0]
    M = x64.T @ y64
    bound = 2.0 ** -(E + 1) * n * np.abs(y64).max(axis=0)[None, :] + (n + n_cells + 8) * 2 * U64 * (np.abs(x64).T @ np.abs(y64))
    return M, bound


def init_state(seed, n, d, n_cells):
    """CodecTrainer.init's seeded choices: -> (T f32, sorted row ids)."""
    rng = np.random.default_rng(seed)
    T = np.linalg.qr(rng.standard_normal((d, d)))[0].astype(np.float32)
    rows = np.sort(rng.choice(n, n_cells, replace=False))
    return T, rows


def adc_error(orc, x, q, cent, T, dpc):
    """E over rows and queries of (q' . (x' - y))^2 in float64 (tests/test_abi_and_host.py's adc_error), codes by the oracle."""
    xr = rotate(orc, T, x)
    y = quantized(assign(orc, xr, cent, dpc), cent, dpc)
    qr = q.astype(np.float64) @ T.astype(np.float64).T
    return float(((qr @ (xr.astype(np.float64) - y.astype(np.float64)).T) ** 2).mean())


def train_f64(orc, x, q, seed, rounds, steps, lr, kmeans_iters, dpc=18, n_cells=256):
    """The whole algorithm with the arithmetic between rotation and assignment in float64: -> (centroids, T, losses per round,
    (centroids, T) right after k-means)."""
    n, d = x.shape
    T, rows = init_state(seed, n, d, n_cells)
    xr = rotate(orc, T, x)
    cent = xr[rows].copy()
    C0 = (q.astype(np.float64).T @ q.astype(np.float64) / q.shape[0]).astype(np.float32)
    for _ in range(kmeans_iters):
        cent = kmeans_step(orc, xr, cent, dpc)[0]
    after_kmeans = (cent.copy(), T.copy())
    m = np.zeros((n_cells, d))
    v = np.zeros((n_cells, d))
    t = 0
    hist = []
    for _ in range(rounds):
        Cm = rotated_moment(orc, T, C0)
        losses = []
        for _ in range(steps):
            codes = assign(orc, xr, cent, dpc)
            L, _, g, _ = loss_and_gradient_f64(xr, codes, cent, Cm, dpc)
            losses.append(L)
            p, m, v = adam_step_f64(cent, m, v, g, t, lr)
            t += 1
            cent = p.astype(np.float32)
        hist.append(losses)
        y = quantized(assign(orc, xr, cent, dpc), cent, dpc)
        u, _, vt = np.linalg.svd(xr.astype(np.float64).T @ y.astype(np.float64))
        T = ((u @ vt).T @ T.astype(np.float64)).astype(np.float32)
        xr = rotate(orc, T, x)
    return cent, T, hist, after_kmeans


def low_rank_sample(n=2048, m=256, d=1152):
    """The low-rank sample of tests/test_abi_and_host.py::test_bench_codec_trainer_lowers_the_query_aware_loss (torch CPU generator,
    seed 0) at n rows and m queries: -> (x, q) float32."""
    import torch
    g = torch.Generator().manual_seed(0)
    basis = torch.randn(48, d, generator=g) * (torch.arange(1, 49).float() ** -0.6).unsqueeze(1)
    x = torch.randn(n, 48, generator=g) @ basis + 0.3 * torch.randn(n, d, generator=g) / d ** 0.5 + 0.5 * torch.randn(1, d, generator=g)
    x = x / x.norm(dim=1, keepdim=True)
    q = x[torch.randperm(n, generator=g)[:m]] + 0.05 * torch.randn(m, d, generator=g) / d ** 0.5
    q = q / q.norm(dim=1, keepdim=True)
    return x.numpy().astype(np.float32), q.numpy().astype(np.float32)
