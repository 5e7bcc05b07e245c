"""Codec training on the device (include/mse.h mse_pq_trainer, csrc/pq_train.hip) against tests/codec_train_ref.py: the
order-free sum and the k-means step bit for bit, the residual GEMM, the loss, the gradient and the cross matrix within bounds that are
derived in the restatement's docstrings, one Adam step against float64, and the whole training on a small low-rank sample."""
import ctypes as C

import numpy as np
import pytest

import codec_train_ref as ref

pytestmark = pytest.mark.gpu

D, DPC, CELLS = 1152, 18, 256


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def device_sum(mse, v, code, n_cells):
    from mse import ffi
    v = np.ascontiguousarray(v, np.float32)
    code = np.ascontiguousarray(code, np.uint8)
    sums = np.full((n_cells, v.shape[1]), -1, np.int64)
    E = C.c_int(-12345)
    ffi.check(ffi.lib().mse_debug_accumulate_by_code(_p(v, C.c_float), v.shape[0], v.shape[1], _p(code, C.c_uint8), n_cells, _p(sums, C.c_int64),
                                                     C.byref(E)), "debug_accumulate_by_code")
    return sums, int(E.value)


def device_gemm(mse, xr, codes, cent, Cm, dpc):
    from mse import ffi
    n, d = xr.shape
    G = np.empty((n, d), np.float32)
    l = np.empty(n, np.float32)
    ffi.check(ffi.lib().mse_debug_residual_gemm(_p(xr, C.c_float), _p(codes, C.c_uint8), _p(cent, C.c_float), _p(Cm, C.c_float), n, d, dpc,
                                                cent.shape[0], _p(G, C.c_float), _p(l, C.c_float)), "debug_residual_gemm")
    return G, l


def random_rotation(seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))[0].astype(np.float32)


def random_moment(seed, rank=64):
    """A random positive semi-definite matrix of trace 1."""
    a = np.random.default_rng(seed).standard_normal((D, rank))
    c = a @ a.T
    return (c / np.trace(c)).astype(np.float32)


def sample_rows(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) / np.sqrt(D) + 0.5 * rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32)


# ---- 1. the order-free sum ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cells", [256, 7])
@pytest.mark.parametrize("w", [18, 36, 1152])
@pytest.mark.parametrize("n", [1, 63, 1000, 4133])
def test_order_free_sum_equals_the_restatement(gpu, mse, n, w, n_cells):
    """Values of both signs with magnitudes from 2^-20 to 1, random cells (256 cells leave some empty at every n here; 4133 rows take two
    workgroups along the rows, 1152 columns 64 along the columns): sums and E equal the numpy restatement bit for bit, twice."""
    rng = np.random.default_rng(1000 * n + w + n_cells)
    v = (rng.uniform(0.5, 1.0, (n, w)) * rng.choice([-1.0, 1.0], (n, w)) * 2.0 ** rng.integers(-20, 1, (n, w))).astype(np.float32)
    v.flat[rng.integers(0, v.size)] = np.float32(-1.0)          # vmax an exact power of two at the top of the range
    code = rng.integers(0, n_cells, n).astype(np.uint8)
    S_ref, E_ref = ref.accumulate_by_code(v, code, n_cells)
    S1, E1 = device_sum(mse, v, code, n_cells)
    S2, E2 = device_sum(mse, v, code, n_cells)
    assert E1 == E_ref == E2
    assert np.array_equal(S1, S_ref)
    assert S1.tobytes() == S2.tobytes()
    if n_cells == 256 and n < 1000:
        assert (np.bincount(code, minlength=256) == 0).any() and not S1[np.bincount(code, minlength=256) == 0].any()


@pytest.mark.parametrize("n,w", [(4133, 18), (1000, 1152)])
def test_order_free_sum_with_every_row_in_one_cell(gpu, mse, n, w):
    rng = np.random.default_rng(n + w)
    v = (rng.standard_normal((n, w)) * 2.0 ** rng.integers(-20, 1, (n, 1))).astype(np.float32)
    code = np.full(n, 3, np.uint8)
    S_ref, E_ref = ref.accumulate_by_code(v, code, 7)
    S, E = device_sum(mse, v, code, 7)
    assert E == E_ref and np.array_equal(S, S_ref)
    assert not S[[0, 1, 2, 4, 5, 6]].any()


def test_order_free_sum_edges(gpu, mse):
    """All-zero input, one tiny value (a subnormal maximum), and a non-finite value, which is refused."""
    z = np.zeros((5, 18), np.float32)
    S, E = device_sum(mse, z, np.zeros(5, np.uint8), 2)
    assert E == ref.fixed_exponent(0.0, 5) and not S.any()
    t = z.copy()
    t[2, 3] = np.float32(2.0 ** -140)
    S, E = device_sum(mse, t, np.array([0, 1, 1, 0, 1], np.uint8), 2)
    S_ref, E_ref = ref.accumulate_by_code(t, np.array([0, 1, 1, 0, 1], np.uint8), 2)
    assert E == E_ref and np.array_equal(S, S_ref) and S[1, 3] != 0
    for bad in (np.inf, -np.inf, np.nan):
        t = z.copy()
        t[4, 17] = bad
        with pytest.raises(mse.MseError, match="non-finite"):
            device_sum(mse, t, np.zeros(5, np.uint8), 2)


# ---- 2. k-means --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dpc,n_cells,n", [(18, 256, 3000), (36, 7, 300)])
def test_kmeans_steps_equal_the_restatement(gpu, mse, orc, dpc, n_cells, n):
    x = sample_rows(11 + n, n)
    T = random_rotation(5)
    xr = ref.rotate(orc, T, x)
    cent0 = xr[np.random.default_rng(3).choice(n, n_cells, replace=False)].copy()
    cent0[5] = cent0[2]                       # a duplicate: first maximum wins, the second copy gets no member
    tr = mse.CodecTrainer(D, dpc, n_cells)
    tr.set_sample(x)
    tr.set_transform(T)
    tr.set_centroids(cent0)
    assert np.array_equal(tr.rotated_rows(np.arange(0, n, 7)), xr[::7])
    assert np.array_equal(tr.codes(), ref.assign(orc, xr, cent0, dpc))
    cent = cent0
    for it in range(3):
        cent, _, empty = ref.kmeans_step(orc, xr, cent, dpc)
        got_empty = tr.kmeans(1)
        got = tr.arrays()[0]
        assert got.tobytes() == cent.tobytes(), f"iteration {it + 1}"
        assert got_empty == empty
        if it == 0:       # the duplicate is empty in every sub-space and stays put (from then on its twin has moved away)
            assert empty >= D // dpc and np.array_equal(got[5], cent0[5]) and not np.array_equal(got[2], cent0[2])
        assert np.array_equal(tr.codes(), ref.assign(orc, xr, cent, dpc))
    again = mse.CodecTrainer(D, dpc, n_cells)
    again.set_sample(x)
    again.set_transform(T)
    again.set_centroids(cent0)
    again.kmeans(3)
    assert again.arrays()[0].tobytes() == cent.tobytes()
    assert np.array_equal(again.arrays()[1], T)


# ---- 3. the residual GEMM ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 129, 300])
def test_residual_gemm_against_float64(gpu, mse, n):
    """|G - G64| <= K 2^-24 sum_k |r_k| |C_kj| with K = 1152: the gamma bound of a length-K fma chain.  l_row = sum_j r_j G_j is formed
    in f32 from the computed G in a fixed tree: |l_row - l64| <= 1.001 (sum_j |r_j| bG_j + K 2^-24 sum_j |r_j| (|G64_j| + bG_j)) -- the
    error of G carried through, plus the gamma bound of a length-K f32 dot product in any order.  With C = I the product is the residual
    itself, every other term of the chain being an exact zero: G equals the f32 subtraction bit for bit."""
    rng = np.random.default_rng(n)
    xr = sample_rows(n, n)
    cent = sample_rows(77, CELLS)
    codes = rng.integers(0, CELLS, (n, D // DPC)).astype(np.uint8)
    Cm = random_moment(9)
    G, l = device_gemm(mse, xr, codes, cent, Cm, DPC)
    R, G64, bG, l64, bl = ref.residual_product_f64(xr, codes, cent, Cm, DPC)
    eg, el = np.abs(G - G64), np.abs(l - l64)
    print(f"n={n}: max |G - G64| / bound = {np.max(eg / bG):.3g}, max |l - l64| / bound = {np.max(el / bl):.3g}")
    assert np.all(eg <= bG)
    assert np.all(el <= bl)
    G2, l2 = device_gemm(mse, xr, codes, cent, Cm, DPC)
    assert G.tobytes() == G2.tobytes() and l.tobytes() == l2.tobytes()
    Gi, _ = device_gemm(mse, xr, codes, cent, np.eye(D, dtype=np.float32), DPC)
    assert np.array_equal(Gi, R)
    # an asymmetric C: a transposed operand would not pass
    Ca = (rng.standard_normal((D, D)) / D).astype(np.float32)
    Ga, _ = device_gemm(mse, xr, codes, cent, Ca, DPC)
    _, Ga64, bGa, _, _ = ref.residual_product_f64(xr, codes, cent, Ca, DPC)
    assert np.all(np.abs(Ga - Ga64) <= bGa)


# ---- 4 - 6: one shared state -------------------------------------------------------------------------------------------------------

N_STATE = 700


@pytest.fixture(scope="module")
def state(orc):
    """A sample of 700 rows, a rotation, centroids (with six duplicates: cells without members), a query moment, and the float64
    loss and gradient of that state."""
    x = sample_rows(21, N_STATE)
    T = random_rotation(6)
    C0 = random_moment(10)
    xr = ref.rotate(orc, T, x)
    cent = xr[np.random.default_rng(4).choice(N_STATE, CELLS, replace=False)].copy()
    cent += (0.01 * np.random.default_rng(5).standard_normal(cent.shape) / np.sqrt(D)).astype(np.float32)
    cent[250:] = cent[:6]
    codes = ref.assign(orc, xr, cent, DPC)
    Cm = ref.rotated_moment(orc, T, C0)
    L, bL, grad, bg = ref.loss_and_gradient_f64(xr, codes, cent, Cm, DPC)
    return dict(x=x, T=T, C0=C0, xr=xr, cent=cent, codes=codes, Cm=Cm, L=L, bL=bL, grad=grad, bg=bg)


def make_trainer(mse, st):
    tr = mse.CodecTrainer(D, DPC, CELLS)
    tr.set_sample(st["x"])
    tr.set_query_moment(st["C0"])
    tr.set_transform(st["T"])
    tr.set_centroids(st["cent"])
    return tr


@pytest.mark.parametrize("t0,chunk_rows", [(0, None), (1, None), (999, None), (999, 256)])
def test_gradient_and_one_adam_step(gpu, mse, state, t0, chunk_rows):
    """One refine step from a state set through the ABI.  The gradient is within the bound of loss_and_gradient_f64 (the GEMM's bound
    summed over a cell's members, plus the fixed-point step).  The update is checked against float64 Adam on the device's own gradient and
    the parameters the ABI received (beta, lr, eps as f32): |update - update64| <= 1e-5 |update64| + ulp(p) -- about ten f32 roundings.
    chunk_rows = 256 takes the rows in three passes of the GEMM (256, 256, 188): same loss bits, gradient within the same bound."""
    from mse import ffi
    st = state
    rng = np.random.default_rng(t0 + 1)
    gs = float(np.sqrt((st["grad"] ** 2).mean()))
    m0 = (gs * rng.standard_normal((CELLS, D))).astype(np.float32) if t0 else np.zeros((CELLS, D), np.float32)
    v0 = (gs * gs * rng.uniform(0.5, 1.5, (CELLS, D))).astype(np.float32) if t0 else np.zeros((CELLS, D), np.float32)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    tr = make_trainer(mse, st)
    if chunk_rows:
        ffi.check(ffi.lib().mse_debug_pq_trainer_chunk_rows(tr._h, chunk_rows), "chunk_rows")
    tr.set_adam_state(m0, v0, t0)
    # mse_pq_trainer_loss changes no state
    L_before = tr.loss()
    assert tr.arrays()[0].tobytes() == st["cent"].tobytes()
    ms, vs, ts = tr.adam_state()
    assert ms.tobytes() == m0.tobytes() and vs.tobytes() == v0.tobytes() and ts == t0
    assert np.array_equal(tr.codes(), st["codes"])
    losses = tr.refine(1, lr=lr, betas=(b1, b2), eps=eps)
    assert len(losses) == 1 and losses[0] == L_before
    print(f"loss {losses[0]!r} float64 {st['L']!r} bound {st['bL']:.3g}")
    assert abs(losses[0] - st["L"]) <= st["bL"]
    g = tr.gradient()
    err = np.abs(g - st["grad"])
    print(f"max |grad - grad64| / bound = {np.max(err[st['bg'] > 0] / st['bg'][st['bg'] > 0]):.3g}")
    assert np.all(err <= st["bg"])
    p1, (m1, v1, t1) = tr.arrays()[0], tr.adam_state()
    assert t1 == t0 + 1
    f = lambda a: float(np.float32(a))
    p64, m64, v64 = ref.adam_step_f64(st["cent"], m0, v0, g, t0, f(lr), f(b1), f(b2), f(eps))
    upd, upd64 = p1.astype(np.float64) - st["cent"].astype(np.float64), p64 - st["cent"].astype(np.float64)
    assert np.all(np.abs(upd - upd64) <= 1e-5 * np.abs(upd64) + np.spacing(np.abs(st["cent"])))
    assert np.all(np.abs(m1 - m64) <= 4 * ref.U32 * (np.abs(f(b1) * m0.astype(np.float64)) + np.abs((1 - f(b1)) * g.astype(np.float64))) + 1e-45)
    assert np.all(np.abs(v1 - v64) <= 6 * ref.U32 * np.abs(v64) + 1e-45)
    # cells without members: zero gradient, moved by their momentum only
    for s in range(D // DPC):
        empty = np.bincount(st["codes"][:, s], minlength=CELLS) == 0
        assert empty[250:].all()
        sl = slice(s * DPC, (s + 1) * DPC)
        assert not g[empty, sl].any()
        if t0:
            assert (upd[empty, sl] != 0).mean() > 0.99      # (an update below half an ulp of its parameter leaves it in place)
        else:
            assert not upd[empty, sl].any()
    if chunk_rows:
        whole = make_trainer(mse, st)
        whole.set_adam_state(m0, v0, t0)
        assert whole.refine(1, lr=lr, betas=(b1, b2), eps=eps)[0] == losses[0]
        assert np.all(np.abs(whole.gradient() - g) <= 2 * st["bg"])


def test_refine_needs_a_query_moment_and_loss_falls(gpu, mse, state):
    st = state
    tr = mse.CodecTrainer(D, DPC, CELLS)
    tr.set_sample(st["x"])
    tr.set_transform(st["T"])
    tr.set_centroids(st["cent"])
    with pytest.raises(mse.MseError, match="query moment"):
        tr.refine(1)
    with pytest.raises(mse.MseError, match="query moment"):
        tr.loss()
    tr.set_query_moment(st["C0"])
    losses = tr.refine(4, lr=1e-3)
    assert len(losses) == 4 and losses[3] < losses[0]
    assert tr.adam_state()[2] == 4
    t = tr.timing()
    assert set(t) == {"assign", "gemm", "accumulate", "adam"} and all(v > 0 for v in t.values())
    pq = tr.quantizer()
    c, T = tr.arrays()
    assert np.array_equal(pq.quantize_batch(st["x"][:50]), tr.codes()[:50])
    with pytest.raises(mse.MseError, match="fewer rows"):
        tr.set_sample(st["x"][:100])


def test_set_transform_rotates_the_original_sample_again(gpu, mse, orc, state):
    """A second set_transform: codes equal the oracle's under the NEW transform applied to the unrotated rows (a rotation of the previous
    X' would differ), and the loss agrees with float64 over the restated T C0 T^T within the loss bound."""
    st = state
    tr = make_trainer(mse, st)
    T2 = random_rotation(8)
    tr.set_transform(T2)
    xr2 = ref.rotate(orc, T2, st["x"])
    codes2 = ref.assign(orc, xr2, st["cent"], DPC)
    assert np.array_equal(tr.codes(), codes2)
    assert not np.array_equal(codes2, ref.assign(orc, ref.rotate(orc, T2, st["xr"]), st["cent"], DPC))
    assert np.array_equal(tr.rotated_rows([0, 699]), xr2[[0, 699]])
    L, bL, _, _ = ref.loss_and_gradient_f64(xr2, codes2, st["cent"], ref.rotated_moment(orc, T2, st["C0"]), DPC)
    got = tr.loss()
    print(f"loss {got!r} float64 {L!r} bound {bL:.3g}")
    assert abs(got - L) <= bL
    assert np.array_equal(tr.arrays()[1], T2)


def test_cross_matrix_and_rotation_update(gpu, mse, orc, state):
    """M against float64 X'^T Y within cross_f64's bound (half a fixed-point unit per row, weighted by the centroid entry, plus float64
    roundings).  After update_rotation the transform is orthogonal to 1e-6 -- its entries are roundings to f32 of an orthogonal matrix,
    2 x 2^-24 per entry of T T^T with rows of unit norm -- and |X P_new - Y|_F <= |X P_old - Y|_F in float64."""
    st = state
    tr = make_trainer(mse, st)
    y = ref.quantized(st["codes"], st["cent"], DPC)
    E = ref.fixed_exponent(np.abs(st["xr"]).max(), N_STATE)
    M64, bM = ref.cross_f64(st["xr"], y, CELLS, E)
    M = tr.cross()
    print(f"max |M - M64| / bound = {np.max(np.abs(M - M64) / bM):.3g}")
    assert np.all(np.abs(M - M64) <= bM)
    assert tr.cross().tobytes() == M.tobytes()
    tr.update_rotation()
    cent_after, T_new = tr.arrays()
    assert cent_after.tobytes() == st["cent"].tobytes()          # the centroids are not refitted
    Tn = T_new.astype(np.float64)
    assert np.abs(Tn @ Tn.T - np.eye(D)).max() <= 1e-6
    x64, y64 = st["x"].astype(np.float64), y.astype(np.float64)
    before = np.linalg.norm(x64 @ st["T"].astype(np.float64).T - y64)
    after = np.linalg.norm(x64 @ Tn.T - y64)
    print(f"|X P - Y|_F {before!r} -> {after!r}")
    assert after <= before
    assert np.array_equal(tr.codes(), ref.assign(orc, ref.rotate(orc, T_new, st["x"]), st["cent"], DPC))


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------

E2E = dict(rounds=2, steps=12, lr=1e-3, kmeans_iters=2, seed=4)


@pytest.fixture(scope="module")
def trained(mse):
    x, q = ref.low_rank_sample(2048, 256)
    tr = mse.CodecTrainer()
    tr.set_sample(x)
    rows = tr.init(E2E["seed"])
    tr.set_queries(q)
    tr.kmeans(E2E["kmeans_iters"])
    after_kmeans = tr.arrays()
    hist = []
    for _ in range(E2E["rounds"]):
        hist.append(tr.refine(E2E["steps"], lr=E2E["lr"]))
        tr.update_rotation()
    return dict(x=x, q=q, tr=tr, rows=rows, after_kmeans=after_kmeans, hist=hist, arrays=tr.arrays())


def test_end_to_end_training(gpu, mse, orc, trained):
    """The low-rank sample of test_bench_codec_trainer_lowers_the_query_aware_loss at 2048 rows and 256 queries, two rounds of twelve steps.
    The float64 restatement (codec_train_ref.train_f64) meets every condition below on this data on the CPU: losses 3.07e-3 -> 1.16e-3 and
    1.40e-3 -> 7.96e-4 (falling at every step), ADC error 3.07e-3 after k-means -> 9.21e-4, |T T^T - I| 1.2e-8."""
    t = trained
    x, q = t["x"], t["q"]
    T0, rows = ref.init_state(E2E["seed"], x.shape[0], D, CELLS)
    assert np.array_equal(rows, t["rows"]) and np.array_equal(T0, t["after_kmeans"][1])
    for r, losses in enumerate(t["hist"]):
        print(f"round {r}: loss {losses[0]!r} -> {losses[-1]!r}")
        assert len(losses) == E2E["steps"] and losses[-1] < losses[0]
    cent, T = t["arrays"]
    e0 = ref.adc_error(orc, x, q, *t["after_kmeans"], DPC)
    e1 = ref.adc_error(orc, x, q, cent, T, DPC)
    print(f"ADC error on the training queries: {e0!r} after k-means -> {e1!r}")
    assert e1 < e0
    Tn = T.astype(np.float64)
    assert np.abs(Tn @ Tn.T - np.eye(D)).max() <= 1e-6
    assert cent.dtype == np.float32 and cent.shape == (CELLS, D) and np.isfinite(cent).all()
    pq = t["tr"].quantizer()
    assert np.array_equal(pq.quantize_batch(x[:300]), orc.PQ(cent, T, DPC, D).quantize_batch(x[:300]))
    blob = mse.opq_msgpack(cent, T, DPC, D)
    assert np.array_equal(mse.ProductQuantizer.from_msgpack(blob).quantize_batch(x[:64]), pq.quantize_batch(x[:64]))


def test_training_is_reproducible(gpu, mse, trained):
    """ProductQuantizer.train runs the same sequence: the same seed gives byte-identical arrays, and the losses it reports are those of the
    step-by-step run."""
    t = trained
    pq, info = mse.ProductQuantizer.train(t["x"], t["q"], **E2E)
    assert info["query_aware_loss_first_last_per_round"] == [v for h in t["hist"] for v in (h[0], h[-1])]
    cent, T = t["arrays"]
    assert np.array_equal(pq.quantize_batch(t["x"][:300]), t["tr"].quantizer().quantize_batch(t["x"][:300]))
    tr = mse.CodecTrainer()
    tr.set_sample(t["x"])
    tr.init(E2E["seed"])
    tr.set_queries(t["q"])
    tr.kmeans(E2E["kmeans_iters"])
    assert tr.arrays()[0].tobytes() == t["after_kmeans"][0].tobytes()
    tr.refine(E2E["steps"], lr=E2E["lr"])
    tr.update_rotation()
    tr.refine(E2E["steps"], lr=E2E["lr"])
    tr.update_rotation()
    c2, T2 = tr.arrays()
    assert c2.tobytes() == cent.tobytes() and T2.tobytes() == T.tobytes()


# ---- 8. from a resident index -------------------------------------------------------------------------------------------------------

def test_sample_from_a_resident_index(gpu, mse, orc):
    n_base, n = 1500, 600
    vecs = mse.VectorList.generate(0x5EED0001, 0, n_base, D)
    rng = np.random.default_rng(12)
    ids = rng.permutation(n_base)[:n].astype(np.uint32)
    ids[17] = ids[3]                                  # a row may be listed twice
    wide = orc.f16_to_f32(vecs.rows(0, n_base))[ids]
    T = random_rotation(13)
    out = []
    for which in ("rows", "host"):
        tr = mse.CodecTrainer()
        if which == "rows":
            tr.set_sample_rows(vecs, ids)
        else:
            tr.set_sample(wide)
        tr.set_transform(T)
        tr.set_centroids(tr.rotated_rows(np.arange(CELLS)))
        tr.kmeans(2)
        out.append(tr.arrays())
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    tr = mse.CodecTrainer()
    s = mse.Searcher(vecs)
    tr.set_sample_rows(s, ids)                        # a searcher's rows serve as well
    bad = ids.copy()
    bad[5] = n_base
    with pytest.raises(mse.MseError, match="not below"):
        tr.set_sample_rows(vecs, bad)
    with pytest.raises(mse.MseError, match="fewer rows"):
        tr.set_sample_rows(vecs, ids[:255])
