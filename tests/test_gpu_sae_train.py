"""Sparse-autoencoder training on the device (csrc/sae_train.hip, csrc/sae_train_api.hip) against tests/sae_train_ref.py's restatement
of the rule, bit for bit: weights, moments, step count, losses and counters.  The moments after the first step are (1 - beta1) g, so
they pin every bit of every gradient.  tests/test_sae_train_host.py shows on the CPU that the restatement is the reference's module
under F.mse_loss and torch.optim.AdamW."""
import functools

import numpy as np
import pytest

import sae_ref
import sae_train_ref as ref

pytestmark = pytest.mark.gpu

# (E, H, K, B, encoder bias): 1152 and 72 take the 16-byte path of the dense pass, 75, 1 and 33 the guarded one; 129 rows are two row
# tiles of the encode; H = 129 and 300 end inside a group of eight feature rows; B = 1 and (1, 2, 1, 3) are the smallest of everything
SHAPES = [(1152, 384, 16, 5, False), (72, 129, 128, 64, True), (75, 300, 16, 129, True), (1, 2, 1, 3, True), (33, 300, 16, 1, False)]
STEPS = 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def case(shape, seed=0, steps=STEPS):
    """(up, up_bias, down, down_bias, x as f16 bits [steps B, E]) of a fresh model's scale (model.py:20-22)"""
    E, H, K, B, bias = shape
    rng = np.random.default_rng(2000 + seed + E + 7 * H)
    up = (rng.uniform(-1, 1, (H, E)) / np.sqrt(E)).astype(np.float32)
    down = np.ascontiguousarray(up.T)
    up_bias = (rng.uniform(-1, 1, H) / np.sqrt(E)).astype(np.float32) if bias else None
    down_bias = (rng.uniform(-1, 1, E) / np.sqrt(H)).astype(np.float32)
    xh = rng.standard_normal((steps * B, E)).astype(np.float16)
    return up, up_bias, down, down_bias, xh.view(np.uint16)


def widen(xbits):
    return np.ascontiguousarray(xbits).view(np.float16).astype(np.float32)


def snapshot(model):
    """every array of a restated run, copied"""
    s = {k: np.array(v) for k, v in model.state().items()}
    s.update(up=model.up.copy(), down=model.down, down_bias=model.down_bias.copy(), counters=model.counters.copy())
    if model.up_bias is not None:
        s["up_bias"] = model.up_bias.copy()
    return s


def device_snapshot(sae, trainer):
    s = {k: np.array(v) for k, v in trainer.state().items()}
    up, down, ub, db = sae.weights()
    s.update(up=up, down=down, down_bias=db, counters=sae.counters())
    if ub is not None:
        s["up_bias"] = ub
    assert s["t"] == trainer.steps
    return s


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        if k == "t":
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (what, k)


@functools.lru_cache(maxsize=None)
def reference(shape, wd):
    """the restated run, one step at a time: ([snapshot after step s], [loss of step s]); computed once per (shape, weight decay)"""
    up, up_bias, down, down_bias, xbits = case(shape)
    B = shape[3]
    model = ref.Model(up, down, up_bias, down_bias, shape[2], weight_decay=wd)
    x = widen(xbits)
    snaps, losses = [], []
    for s in range(STEPS):
        losses.append(ref.step(model, x[s * B:(s + 1) * B]))
        snaps.append(snapshot(model))
    return snaps, losses


def pair_of(mse, shape, wd=0.0, **kw):
    up, up_bias, down, down_bias, _ = case(shape)
    sae = mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=shape[2])
    return sae, mse.SaeTrainer(sae, weight_decay=wd, **kw)


# ---- the rule, shape by shape ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", SHAPES)
def test_three_steps_are_the_restated_rule(gpu, mse, shape, wd):
    _, _, _, _, xbits = case(shape)
    snaps, losses = reference(shape, wd)
    assert all(l is not None for l in losses)
    B = shape[3]
    sae, tr = pair_of(mse, shape, wd)
    for s in range(STEPS):
        loss = tr.step(xbits, np.arange(s * B, (s + 1) * B))
        assert loss == losses[s], (s, loss, losses[s])
        assert_same(device_snapshot(sae, tr), snaps[s], "after step %d" % (s + 1))
    assert snaps[0]["m_up"].any() and snaps[0]["m_down"].any()     # the first step's moments are (1 - beta1) g


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def run_both(mse, up, up_bias, down, down_bias, K, batches, wd=0.0, **kw):
    """the same batches (f16 bit arrays) through the device and the restatement -> (sae, trainer, restated model, pairs of each step)"""
    sae = mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=K)
    tr = mse.SaeTrainer(sae, weight_decay=wd, **kw)
    model = ref.Model(up, down, up_bias, down_bias, K, weight_decay=wd, **kw)
    pairs = []
    for xb in batches:
        x = widen(xb)
        pairs.append(ref.gradients(model, x)[2])
        want = ref.step(model, x)
        assert tr.step(xb, np.arange(xb.shape[0])) == want
        assert_same(device_snapshot(sae, tr), snapshot(model), "after step %d" % model.t)
    return sae, tr, model, pairs


def test_first_and_last_feature_a_feature_in_every_row_and_an_empty_row(gpu, mse):
    E, H, K, B = 8, 40, 3, 9
    rng = np.random.default_rng(5)
    up = (rng.standard_normal((H, E)) / 4).astype(np.float32)
    up[0] = 1.0                                            # positive rows: feature 0 is every row's largest
    up[H - 1] = 0.0
    up[H - 1, 0] = 6.0                                     # feature H - 1 follows component 0
    down = np.ascontiguousarray(up.T)
    down_bias = rng.standard_normal(E).astype(np.float32) / 8
    x1 = np.abs(rng.standard_normal((B, E))).astype(np.float16) + np.float16(0.25)
    x2 = x1.copy()
    x2[4] = 0                                              # no bias: every pre-activation is 0 and nothing is kept
    batches = [x1.view(np.uint16), x2.view(np.uint16)]
    _, _, _, pairs = run_both(mse, up, None, down, down_bias, K, batches)
    rows, fs = pairs[0]
    assert np.array_equal(np.sort(rows[fs == 0]), np.arange(B)) and (fs == H - 1).any()
    rows, fs = pairs[1]
    assert not (rows == 4).any() and (np.bincount(rows, minlength=B)[np.arange(B) != 4] == K).all()


def test_a_batch_that_keeps_nothing_moves_the_decoder_bias_alone(gpu, mse):
    shape = SHAPES[2]
    up, up_bias, down, down_bias, _ = case(shape)
    zero = np.zeros((4, shape[0]), np.uint16)
    sae, tr, model, pairs = run_both(mse, up, None, down, down_bias, shape[2], [zero])
    assert pairs[0][0].size == 0
    got_up, got_down, _, got_db = sae.weights()
    assert np.array_equal(bits(got_up), bits(up)) and np.array_equal(bits(got_down), bits(down))
    assert not np.array_equal(bits(got_db), bits(down_bias)) and not sae.counters().any()


def test_the_same_id_twice_in_one_batch(gpu, mse):
    shape = (64, 129, 8, 6, True)
    up, up_bias, down, down_bias, xbits = case(shape)
    ids = np.array([3, 1, 3, 0, 5, 3], np.uint32)
    sae, tr = pair_of(mse, shape)
    model = ref.Model(up, down, up_bias, down_bias, shape[2])
    want = ref.step(model, widen(xbits[ids]))
    assert tr.step(mse.VectorList.from_f16s(xbits, shape[0]), ids) == want
    assert_same(device_snapshot(sae, tr), snapshot(model))


def test_batch_times_top_k_at_the_limit_and_one_row_more(gpu, mse):
    E, H, K, B = 4, 300, 256, 256
    rng = np.random.default_rng(9)
    up = (rng.standard_normal((H, E)) / 2).astype(np.float32)
    up_bias = (rng.standard_normal(H) * 0.5 + 3.0).astype(np.float32)      # most units positive: rows keep top_k features
    down = np.ascontiguousarray(up.T)
    down_bias = np.zeros(E, np.float32)
    xh = rng.standard_normal((B + 1, E)).astype(np.float16).view(np.uint16)
    sae = mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=K)
    tr = mse.SaeTrainer(sae)
    with pytest.raises(mse.ffi.MseError, match="exceeds 65536"):
        tr.step(xh, np.arange(B + 1))
    assert tr.steps == 0
    model = ref.Model(up, down, up_bias, down_bias, K)
    want = ref.step(model, widen(xh[:B]))
    assert model.counters.sum() > 60000
    assert tr.step(xh, np.arange(B)) == want
    assert_same(device_snapshot(sae, tr), snapshot(model))


def test_momentum_without_gradient(gpu, mse):
    """feature 2 fires at step 1 only; at steps 2 and 3 its rows of up and down move by their momentum, as torch's AdamW moves them"""
    E, H, K, B = 4, 6, 1, 2
    up = np.zeros((H, E), np.float32)
    up[2, 0], up[4, 1], up[5, 2] = 1.0, 1.0, 0.5
    down = np.ascontiguousarray(up.T) * np.float32(0.5)
    down_bias = np.zeros(E, np.float32)
    first = np.array([[2, 0, 0.5, 0], [3, 0, 0.5, 0.25]], np.float16)      # feature 2 is largest, feature 5 the threshold
    later = np.array([[0, 2, 0.5, 0], [0, 3, 0.5, 0.25]], np.float16)      # feature 4 is
    batches = [first.view(np.uint16), later.view(np.uint16), later.view(np.uint16)]
    sae = mse.SparseAutoencoder(up, down, None, down_bias, top_k=K)
    tr = mse.SaeTrainer(sae, lr=1e-2)
    model = ref.Model(up, down, None, down_bias, K, lr=1e-2)
    seen = []
    for s, xb in enumerate(batches):
        fs = ref.gradients(model, widen(xb))[2][1]
        assert (2 in fs) == (s == 0)
        assert tr.step(xb, np.arange(B)) == ref.step(model, widen(xb))
        assert_same(device_snapshot(sae, tr), snapshot(model))
        seen.append(sae.weights()[0][2].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ---- cuts, resumption, repetition ------------------------------------------------------------------------------------------------------
CUT_SHAPE = (64, 300, 16, 7, True)


def test_cut_resume_and_ids_give_the_same_bytes(gpu, mse):
    shape = CUT_SHAPE
    up, up_bias, down, down_bias, xbits = case(shape, steps=6)
    B, n = shape[3], 6 * shape[3]
    ids = np.arange(n)
    # one call of six steps, against the restatement
    sae, tr = pair_of_case(mse, shape, 6, wd=0.01)
    losses = tr.train(xbits, ids, B)
    model = ref.Model(up, down, up_bias, down_bias, shape[2], weight_decay=0.01)
    want_losses = ref.train(model, widen(xbits), B)
    assert np.array_equal(bits(losses), bits(want_losses)) and tr.steps == 6
    whole = device_snapshot(sae, tr)
    assert_same(whole, snapshot(model))
    # a ragged tail is dropped (train.py:88)
    sae2, tr2 = pair_of_case(mse, shape, 6, wd=0.01)
    assert tr2.train(xbits, np.arange(3 * B + B - 1), B).size == 3 and tr2.steps == 3
    # ... then state and weights into a fresh model and trainer, and three more steps
    up3, down3, ub3, db3 = sae2.weights()
    sae3 = mse.SparseAutoencoder(up3, down3, ub3, db3, top_k=shape[2])
    tr3 = mse.SaeTrainer(sae3, weight_decay=0.01)
    tr3.load_state(tr2.state())
    assert tr3.steps == 3
    more = tr3.train(xbits, ids[3 * B:], B)
    assert np.array_equal(bits(more), bits(want_losses[3:]))
    resumed = device_snapshot(sae3, tr3)
    resumed["counters"] = resumed["counters"] + sae2.counters()           # counters belong to the model, not to the optimizer state
    assert_same(resumed, whole, "resumed")
    # six calls of one step
    sae4, tr4 = pair_of_case(mse, shape, 6, wd=0.01)
    one = [tr4.step(xbits, ids[s * B:(s + 1) * B]) for s in range(6)]
    assert np.array_equal(bits(np.array(one)), bits(want_losses))
    assert_same(device_snapshot(sae4, tr4), whole, "six calls")
    # ids through a base, in another order than the rows lie in
    perm = np.random.default_rng(1).permutation(n)
    base = mse.VectorList.from_f16s(np.ascontiguousarray(xbits[perm]), shape[0])
    sae5, tr5 = pair_of_case(mse, shape, 6, wd=0.01)
    assert np.array_equal(bits(tr5.train(base, np.argsort(perm), B)), bits(want_losses))
    assert_same(device_snapshot(sae5, tr5), whole, "through a base")


def pair_of_case(mse, shape, steps, wd=0.0):
    up, up_bias, down, down_bias, _ = case(shape, steps=steps)
    sae = mse.SparseAutoencoder(up, down, up_bias, down_bias, top_k=shape[2])
    return sae, mse.SaeTrainer(sae, weight_decay=wd)


def test_repetition_and_the_touched_row_skip(gpu, mse):
    shape = (72, 1000, 4, 8, False)                        # 96 pairs a step at most: most of the 1000 features never fire
    _, _, _, _, xbits = case(shape)
    runs = []
    for skip in (True, True, False):
        sae, tr = pair_of(mse, shape)
        tr.set_skip(skip)
        losses = tr.train(xbits, np.arange(xbits.shape[0]), shape[3])
        runs.append((losses, device_snapshot(sae, tr)))
    assert (runs[0][1]["counters"] == 0).sum() > 500
    for losses, snap in runs[1:]:
        assert np.array_equal(bits(losses), bits(runs[0][0]))
        assert_same(snap, runs[0][1])
    snaps, losses = reference_for(shape)
    assert_same(runs[0][1], snaps)
    assert np.array_equal(bits(runs[0][0]), bits(losses))


def reference_for(shape):
    up, up_bias, down, down_bias, xbits = case(shape)
    model = ref.Model(up, down, up_bias, down_bias, shape[2])
    losses = ref.train(model, widen(xbits), shape[3])
    return snapshot(model), losses


# ---- the model after training ------------------------------------------------------------------------------------------------------------
def test_encode_after_training_and_a_table_from_before(gpu, mse):
    shape = CUT_SHAPE
    up, up_bias, down, down_bias, xbits = case(shape)
    sae, tr = pair_of(mse, shape)
    before = sae.encode(xbits[:5], count=False)
    assert before.sq_errors().shape == (5,)
    tr.train(xbits, np.arange(xbits.shape[0]), shape[3])
    with pytest.raises(mse.ffi.MseError, match="another model"):
        before.reconstruct()
    got = sae.encode(xbits[:9], count=False)
    w = sae.weights()
    fresh = mse.SparseAutoencoder(*w, top_k=shape[2]).encode(xbits[:9], count=False)
    model = ref.Model(up, down, up_bias, down_bias, shape[2])
    ref.train(model, widen(xbits), shape[3])
    want = sae_ref.encode(model.up, widen(xbits[:9]), shape[2], model.up_bias)
    for table in (got, fresh):
        c, f, a = table.to_host()
        assert np.array_equal(c, want[0]) and np.array_equal(f, want[1]) and np.array_equal(bits(a), bits(want[2]))
    assert np.array_equal(bits(got.sq_errors()), bits(fresh.sq_errors()))
    assert np.array_equal(sae.feature_queries([0, 1]), np.ascontiguousarray(model.down[:, [0, 1]].T.astype(np.float16)).view(np.uint16))


def test_a_refused_step_changes_nothing_and_the_handle_trains_on(gpu, mse):
    shape = CUT_SHAPE
    up, up_bias, down, down_bias, xbits = case(shape)
    B = shape[3]
    bad = xbits.copy()
    bad[B + 2, 5] = 0x7E00                                  # a NaN in the second step's batch
    sae, tr = pair_of(mse, shape)
    with pytest.raises(mse.StepRefused) as info:
        tr.train(bad, np.arange(3 * B), B)
    model = ref.Model(up, down, up_bias, down_bias, shape[2])
    want = ref.train(model, widen(bad), B)
    assert want.size == 1 and info.value.steps_done == 1 and np.array_equal(bits(info.value.losses), bits(want))
    assert tr.steps == 1
    assert_same(device_snapshot(sae, tr), snapshot(model), "after the refused call")
    losses = tr.train(xbits, np.arange(B, 3 * B), B)
    assert np.array_equal(bits(losses), bits(ref.train(model, widen(xbits[B:]), B)))
    assert_same(device_snapshot(sae, tr), snapshot(model), "after training on")
    # an infinite row: a non-finite loss
    inf = xbits.copy()
    inf[0, 0] = 0x7C00
    with pytest.raises(mse.StepRefused) as info:
        tr.step(inf, np.arange(B))
    assert info.value.steps_done == 0 and ref.step(model, widen(inf[:B])) is None
    assert_same(device_snapshot(sae, tr), snapshot(model), "after the infinite row")


def test_errors_leave_the_handles_usable(gpu, mse):
    shape = CUT_SHAPE
    up, up_bias, down, down_bias, xbits = case(shape)
    B = shape[3]
    sae, tr = pair_of(mse, shape)
    base = mse.VectorList.from_f16s(xbits, shape[0])
    with pytest.raises(mse.ffi.MseError, match="components"):
        tr.step(np.zeros((B, 128), np.uint16), np.arange(B))
    with pytest.raises(mse.ffi.MseError, match="not below"):
        tr.step(base, np.array([0, 1, xbits.shape[0]], np.uint32))
    with pytest.raises(mse.ffi.MseError, match="down_bias"):
        mse.SaeTrainer(mse.SparseAutoencoder(up, down, up_bias, None, top_k=shape[2]))
    with pytest.raises(mse.ffi.MseError, match="AdamW"):
        mse.SaeTrainer(sae, betas=(1.0, 0.999))
    assert tr.steps == 0 and not sae.counters().any()
    model = ref.Model(up, down, up_bias, down_bias, shape[2])
    assert tr.step(base, np.arange(B)) == ref.step(model, widen(xbits[:B]))
    assert_same(device_snapshot(sae, tr), snapshot(model))
    # a model freed before its trainer: the trainer refuses, and freeing it is safe
    sae.close()
    with pytest.raises(mse.ffi.MseError, match="freed"):
        tr.step(base, np.arange(B))
    with pytest.raises(mse.ffi.MseError, match="freed"):
        tr.state()
    tr.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_planted_directions_are_learnt(gpu, mse):
    """rows: sparse non-negative combinations of 24 planted unit directions in 32 dimensions.  200 steps: the device's losses are the
    restatement's, and the held-out error falls"""
    E, H, K, B, steps, planted = 32, 128, 4, 64, 200, 24
    rng = np.random.default_rng(17)
    dirs = rng.standard_normal((planted, E))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)

    def draw(n):
        coef = np.where(rng.random((n, planted)) < 3.0 / planted, rng.uniform(0.5, 1.5, (n, planted)), 0.0)
        return (coef @ dirs).astype(np.float16).view(np.uint16)

    train_rows, held_out = draw(steps * B), draw(512)
    sae = mse.SparseAutoencoder.random(E, H, K, seed=3)
    assert sae.d_emb == E and sae.d_hidden == H and np.array_equal(sae.weights()[1], sae.weights()[0].T)
    up, down, ub, db = sae.weights()
    mse_before = sae.encode(held_out, count=False).mse()
    tr = mse.SaeTrainer(sae, lr=1e-2)
    losses = tr.train(train_rows, np.arange(steps * B), B)
    model = ref.Model(up, down, ub, db, K, lr=1e-2)
    want = ref.train(model, widen(train_rows), B)
    assert want.size == steps and np.array_equal(bits(losses), bits(want))
    mse_after = sae.encode(held_out, count=False).mse()
    print("sae training, planted directions: held-out mse %.6g before, %.6g after %d steps; first loss %.6g, last %.6g"
          % (mse_before, mse_after, steps, losses[0], losses[-1]))
    assert mse_after < mse_before
