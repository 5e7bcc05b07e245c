"""The ensemble rater on the device (csrc/rater.hip, csrc/rater_api.hip) against tests/rater_ref.py's restatement of the rule, bit for
bit: weights, moments, step count, member scores and pair variances; the losses within a bound.  The moments after the first step are
(1 - beta1) g, so they pin every bit of every gradient.  tests/test_rater_host.py shows on the CPU that the restatement is the
reference's module under F.binary_cross_entropy and AdamW."""
import functools

import numpy as np
import pytest

import rater_ref as ref

pytestmark = pytest.mark.gpu

# (E, M, C, B): 1152 is the shipped width, the 16-byte path of the dense pass and batch 1; 72 the largest batch; 75 the guarded path;
# (1, 1, 1, 1) the smallest of everything; (33, 16, 8, 2) the most channels with members off every tile boundary; 128 members exactly
# on tile boundaries
SHAPES = [(1152, 2, 3, 1), (72, 3, 3, 64), (75, 2, 1, 5), (1, 1, 1, 1), (33, 16, 8, 2), (128, 3, 2, 3)]
STEPS = 3
N_ROWS = 40
LOG_ULPS = 1   # OCML documents its f64 log at 1 ulp; numpy's is taken at the same


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def widen(xbits):
    return np.ascontiguousarray(xbits).view(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape, steps=STEPS):
    """(up, bias, down, rows as f16 bits [N_ROWS, E], pair ids [steps, M, B, 2], targets [steps, M, B, C]) of a fresh ensemble's scale;
    down is four times nn.Linear's so that the head works off its linear part"""
    E, M, C, B = shape
    rng = np.random.default_rng(3000 + E + 7 * M)
    up, bias, down = ref.random_weights(E, M, C, rng)
    down = (down * 4).astype(np.float32)
    rows = rng.standard_normal((N_ROWS, E)).astype(np.float16).view(np.uint16)
    ids = rng.integers(0, N_ROWS, (steps, M, B, 2)).astype(np.uint32)
    y = rng.choice([0.1, 0.3, 0.5, 0.7, 0.9], (steps, M, B, C)).astype(np.float32)
    return up, bias, down, rows, ids, y


def snapshot(model):
    s = {k: np.array(v) for k, v in model.state().items()}
    s.update(up=model.up.copy(), bias=model.bias.copy(), down=model.down.copy())
    return s


def device_snapshot(rater, trainer):
    s = {k: np.array(v) for k, v in trainer.state().items()}
    up, bias, down = rater.weights()
    s.update(up=up, bias=bias, down=down)
    assert s["t"] == trainer.steps
    return s


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in want:
        if k == "t":
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def loss_bound(shape, loss):
    """|device - restatement| for a loss: both sum N = M B C non-negative terms of two non-negative products each in one order, so the
    relative errors add up and none is amplified: two logs per term on either side, each within LOG_ULPS ulps = 2 LOG_ULPS 2^-53
    relative, and per side a multiply, an add, the chain of N - 1 adds and the divide"""
    _, M, C, B = shape
    n = M * B * C
    return (4 * LOG_ULPS + 2 * (n + 2)) * 2.0 ** -53 * abs(loss)


@functools.lru_cache(maxsize=None)
def reference(shape, wd, steps=STEPS):
    """the restated run, one step at a time: ([snapshot after step s], [loss of step s]); computed once per (shape, weight decay)"""
    up, bias, down, rows, ids, y = case(shape, steps)
    model = ref.Model(up, bias, down, shape[1], weight_decay=wd)
    x = widen(rows)
    snaps, losses = [], []
    for s in range(steps):
        losses.append(ref.step(model, ref.slots_of(x, ids[s]), y[s]))
        snaps.append(snapshot(model))
    return snaps, losses


def pair_of(mse, shape, wd=0.0, steps=STEPS, **kw):
    up, bias, down = case(shape, steps)[:3]
    rater = mse.Rater.from_wide(up, bias, down, shape[1])
    return rater, mse.RaterTrainer(rater, weight_decay=wd, **kw)


# ---- the rule, shape by shape ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", SHAPES)
def test_three_steps_are_the_restated_rule(gpu, mse, shape, wd):
    _, _, _, rows, ids, y = case(shape)
    snaps, losses = reference(shape, wd)
    assert all(l is not None for l in losses)
    rater, tr = pair_of(mse, shape, wd)
    for s in range(STEPS):
        loss = float(tr.run(rows, ids[s:s + 1], y[s:s + 1])[0])
        print("loss of step %d: device %.17g restatement %.17g bound %.3g" % (s, loss, losses[s], loss_bound(shape, losses[s])))
        assert abs(loss - losses[s]) <= loss_bound(shape, losses[s]), (s, loss, losses[s])
        assert_same(device_snapshot(rater, tr), snaps[s], "after step %d" % (s + 1))
    assert snaps[0]["m_up"].any() and snaps[0]["m_bias"].any() and snaps[0]["m_down"].any()     # the first step's moments are (1 - beta1) g


# ---- cutting ----------------------------------------------------------------------------------------------------------------------------
def test_a_run_is_the_same_bytes_however_it_is_cut(gpu, mse):
    shape, steps = (64, 3, 2, 4), 6                           # a base's width is a multiple of 64
    _, _, _, rows, ids, y = case(shape, steps)
    snaps, losses = reference(shape, 0.01, steps)

    def whole():
        rater, tr = pair_of(mse, shape, 0.01, steps)
        got = tr.run(rows, ids, y)
        return device_snapshot(rater, tr), got

    a, losses_a = whole()
    assert_same(a, snaps[-1], "one call of six steps")
    assert all(abs(l - w) <= loss_bound(shape, w) for l, w in zip(losses_a, losses))
    b, losses_b = whole()
    assert_same(b, a, "a second run")
    assert np.array_equal(losses_a, losses_b)
    rater, tr = pair_of(mse, shape, 0.01, steps)
    singly = [float(tr.run(rows, ids[s:s + 1], y[s:s + 1])[0]) for s in range(steps)]
    assert_same(device_snapshot(rater, tr), a, "six calls of one step")
    assert np.array_equal(singly, losses_a)
    # three steps, then the state and the weights into a fresh rater and trainer, then three more
    rater, tr = pair_of(mse, shape, 0.01, steps)
    tr.run(rows, ids[:3], y[:3])
    assert_same(device_snapshot(rater, tr), snaps[2], "after three steps")
    rater2 = mse.Rater.from_wide(*rater.weights(), shape[1])
    tr2 = mse.RaterTrainer(rater2, weight_decay=0.01)
    tr2.load_state(tr.state())
    assert tr2.steps == 3
    tail = tr2.run(rows, ids[3:], y[3:])
    assert_same(device_snapshot(rater2, tr2), a, "three steps, a fresh pair, three more")
    assert np.array_equal(tail, losses_a[3:])
    # ids through a base against host rows
    vecs = mse.VectorList.from_f16s(rows, shape[0])
    rater, tr = pair_of(mse, shape, 0.01, steps)
    via_base = tr.run(vecs, ids, y)
    assert_same(device_snapshot(rater, tr), a, "ids through a base")
    assert np.array_equal(via_base, losses_a)


def test_train_draws_one_permutation_per_member_and_runs_the_ragged_batch(gpu, mse):
    """RaterTrainer.train (train.py:114-119) against the same permutations handed to run; 7 pairs in batches of 3: two whole steps and
    one of a single pair per epoch"""
    shape = (33, 2, 1, 3)
    up, bias, down, rows, _, _ = case(shape)
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, N_ROWS, (7, 2)).astype(np.uint32)
    ratings = np.stack([mse.map_rating(r) for r in ("1", "2", "1+", "2p", "eq", "1", "2+")]).astype(np.float32)
    assert ratings[:, 0].tolist() == [np.float32(v) for v in (0.9, 0.1, 0.7, 0.3, 0.5, 0.9, 0.3)]
    rater, tr = pair_of(mse, shape)
    losses = tr.train(rows, pairs, ratings, 2, np.random.default_rng(77), batch_size=3)
    assert losses.shape == (6,) and tr.steps == 6
    model = ref.Model(up, bias, down, shape[1])
    x, rng2 = widen(rows), np.random.default_rng(77)
    for _ in range(2):
        orders = np.stack([rng2.permutation(7) for _ in range(shape[1])])
        for lo, hi in ((0, 3), (3, 6), (6, 7)):
            o = orders[:, lo:hi]
            assert ref.step(model, ref.slots_of(x, pairs[o]), ratings[o]) is not None
    assert_same(device_snapshot(rater, tr), snapshot(model), "two epochs")
    # the graph's forwarders keep no state of their own
    rater2, tr2 = pair_of(mse, shape)
    mse.DeviceGraph.train_rater(None, tr2, rows, pairs, ratings, 2, np.random.default_rng(77), 3)
    assert_same(device_snapshot(rater2, tr2), snapshot(model), "through DeviceGraph.train_rater")


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def test_a_row_against_itself_a_row_in_many_slots_and_hard_targets(gpu, mse):
    shape = (33, 2, 2, 3)
    up, bias, down, rows, _, _ = case(shape)
    ids = np.array([[[[5, 5], [5, 7], [7, 5]], [[5, 5], [7, 7], [5, 9]]]], np.uint32)          # [1, M, B, 2]
    y = np.array([[[[0.0, 1.0], [1.0, 0.0], [0.5, 0.0]], [[1.0, 1.0], [0.0, 0.0], [0.9, 1.0]]]], np.float32)
    model = ref.Model(up, bias, down, shape[1])
    x = widen(rows)
    got = ref.gradients(model, ref.slots_of(x, ids[0]), y[0])
    assert not (got[2][:, 0] - got[2][:, 1]).any()                                       # z = 0 exactly where a row meets itself
    rater, tr = pair_of(mse, shape)
    for _ in range(2):
        want = ref.step(model, ref.slots_of(x, ids[0]), y[0])
        loss = float(tr.run(rows, ids, y)[0])
        assert abs(loss - want) <= loss_bound(shape, want)
        assert_same(device_snapshot(rater, tr), snapshot(model))


def test_batch_limit(gpu, mse):
    shape = (8, 1, 1, 1)
    rater, tr = pair_of(mse, shape)
    rows = case(shape)[3]
    ok = np.zeros((1, 1, 64, 2), np.uint32)
    ok[..., 1] = 1
    assert tr.run(rows, ok, np.full((1, 1, 64, 1), 0.5, np.float32)).shape == (1,) and tr.steps == 1
    before = device_snapshot(rater, tr)
    with pytest.raises(mse.MseError, match="65"):
        tr.run(rows, np.zeros((1, 1, 65, 2), np.uint32), np.full((1, 1, 65, 1), 0.5, np.float32))
    assert_same(device_snapshot(rater, tr), before)


@pytest.mark.parametrize("bad_bits", [0x7E00, 0x7C00, 0xFC00], ids=["nan", "inf", "-inf"])
def test_a_non_finite_row_refuses_the_step_and_the_rest_of_the_call(gpu, mse, bad_bits):
    shape = (75, 2, 1, 5)
    up, bias, down, rows, ids, y = case(shape)
    snaps, _ = reference(shape, 0.0)
    bad = rows.copy()
    bad_row = N_ROWS                                          # a row only step 1 names
    bad = np.concatenate([bad, rows[:1]])
    bad[bad_row, 74] = bad_bits
    ids2 = ids.copy()
    ids2[1, 1, 4, 1] = bad_row
    rater, tr = pair_of(mse, shape)
    with pytest.raises(mse.StepRefused) as e:
        tr.run(bad, ids2, y)
    assert e.value.steps_done == 1 and len(e.value.losses) == 1 and tr.steps == 1
    assert_same(device_snapshot(rater, tr), snaps[0], "after the refusal")       # everything as step 0 left it
    tr.run(bad, ids[1:], y[1:])                                                   # the same handles go on
    assert_same(device_snapshot(rater, tr), snaps[2], "after going on")


def test_a_freed_rater_and_a_width_mismatch_are_errors(gpu, mse):
    shape = (33, 2, 1, 5)
    up, bias, down, rows, ids, y = case(shape)
    rater, tr = pair_of(mse, shape)
    wrong = mse.VectorList.from_f16s(np.zeros((4, 64), np.uint16), 64)
    with pytest.raises(mse.MseError, match="d_emb"):
        tr.run(wrong, np.zeros_like(ids), y)
    with pytest.raises(mse.MseError, match="d_emb"):
        rater.member_scores(wrong)
    with pytest.raises(mse.MseError, match="not below"):
        tr.run(rows, ids + np.uint32(N_ROWS), y)
    assert tr.steps == 0
    tr.run(rows, ids[:1], y[:1])
    rater.close()
    with pytest.raises(mse.MseError, match="freed"):
        tr.run(rows, ids[:1], y[:1])
    with pytest.raises(mse.MseError, match="freed"):
        tr.state()
    with pytest.raises(mse.MseError, match="dropout"):
        mse.RaterTrainer(rater, dropout=0.1)


# ---- member scores and disagreement -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def score_case(E):
    M, C, n = 3, 2, 129
    rng = np.random.default_rng(40 + E)
    up, bias, down = ref.random_weights(E, M, C, rng)
    down = (down * 4).astype(np.float32)
    rows = rng.standard_normal((n, E)).astype(np.float16).view(np.uint16)
    return up, bias, down, rows, ref.member_scores(ref.Model(up, bias, down, M), widen(rows))


@pytest.mark.parametrize("E", [75, 128])
def test_member_scores_are_the_restated_scores_however_they_are_asked_for(gpu, mse, E):
    up, bias, down, rows, want = score_case(E)
    rater = mse.Rater.from_wide(up, bias, down, 3)
    sources = (rows, mse.VectorList.from_f16s(rows, E)) if E % 64 == 0 else (rows,)      # a base's width is a multiple of 64
    vecs = sources[-1]
    for n in (1, 127, 129):
        for source in sources:
            t = rater.member_scores(source, n=n)
            assert len(t) == n and np.array_equal(bits(t.to_host()), bits(want[:n])), n
    ids = np.array([128, 0, 5, 5, 127, 64, 128], np.uint32)
    for source in sources:
        assert np.array_equal(bits(rater.member_scores(source, ids=ids).to_host()), bits(want[ids]))
        assert np.array_equal(bits(rater.member_scores(source, first=5, n=100).to_host()), bits(want[5:105]))
    assert len(rater.member_scores(vecs, first=129)) == 0
    with pytest.raises(mse.MseError):
        rater.member_scores(vecs, first=100, n=30)
    # what the trainer's forward pass makes of the same rows
    tr = mse.RaterTrainer(rater)
    pair_ids = np.array([[[[0, 128], [5, 5], [64, 1]], [[127, 2], [128, 0], [3, 3]], [[9, 8], [7, 6], [5, 4]]]], np.uint32)
    tr.run(vecs, pair_ids, np.full((1, 3, 3, 2), 0.7, np.float32))
    s = tr.last_scores()                                       # [M, 2 B, C], made before the update
    slots = pair_ids[0].reshape(3, 6)
    for m in range(3):
        assert np.array_equal(bits(s[m]), bits(want[slots[m], m])), m


def test_pair_variance_and_top_pairs(gpu, mse):
    up, bias, down, rows, want = score_case(75)
    rater = mse.Rater.from_wide(up, bias, down, 3)
    table = rater.member_scores(rows)
    rng = np.random.default_rng(6)
    a, b = rng.integers(0, 129, 300), rng.integers(0, 129, 300)
    a[:3] = b[:3]                                              # a row with itself: variance +0
    a[10:14], b[10:14] = a[20:24], b[20:24]                    # ties
    var = table.pair_variance(a, b)
    want_var = ref.pair_variance(want, a, b)
    assert np.array_equal(bits(var), bits(want_var)) and not bits(var[:3]).any()
    order, top = table.top_pairs(a, b, 40)
    assert np.array_equal(order, ref.top_pairs(want_var, 40)) and np.array_equal(bits(top), bits(want_var[order]))
    assert len(table.top_pairs(a, b, 1000)[0]) == 300
    g_order, g_top = mse.DeviceGraph.rate_pairs(None, rater, rows, a, b, 40)
    assert np.array_equal(g_order, order) and np.array_equal(bits(g_top), bits(top))
    with pytest.raises(mse.MseError, match="not below"):
        table.pair_variance([0, 129], [1, 1])
    single = mse.Rater.from_wide(up[:75], bias[:75], down[:, :75], 1)
    with pytest.raises(mse.MseError, match="one member"):
        single.member_scores(rows, n=4).pair_variance([0], [1])


# ---- export ------------------------------------------------------------------------------------------------------------------------------
def test_exported_score_model_scores_the_member_mean(gpu, mse):
    up, bias, down, rows, want = score_case(128)
    rater = mse.Rater.from_wide(up, bias, down, 3)
    got = rater.to_score_model().score_rows(mse.VectorList.from_f16s(rows, 128)).to_host()
    assert np.allclose(got, want.astype(np.float64).mean(axis=1), rtol=1e-5, atol=1e-5)
    fresh = mse.Rater.random(16, 4, 3, np.random.default_rng(1))
    u, b, d = fresh.weights()
    assert u.shape == (64, 16) and b.shape == (64,) and d.shape == (3, 64) and max(np.abs(u).max(), np.abs(b).max(), np.abs(d).max()) <= 0.25
    with pytest.raises(mse.MseError, match="dropout"):
        mse.Rater.random(16, 4, 3, np.random.default_rng(1), dropout=0.1)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_planted_utility_end_to_end(gpu, mse):
    """A hidden direction in E = 32, ratings 0.9 / 0.1 by the sign of the utility difference, M = 4, C = 1, B = 1, 300 steps at lr 2e-3:
    on 256 held-out pairs the restatement alone takes the loss from 0.6945 to 0.4939 and the share of correctly ordered pairs from 0.539
    to 0.879; the device's weights equal the restatement's bit for bit."""
    c, P = ref.planted_case(), ref.PLANTED
    before, after, model = ref.planted_run()
    assert after[0] < before[0] - 0.05 and after[1] > before[1] + 0.2 and after[1] > 0.8
    rater = mse.Rater.from_wide(c["up"], c["bias"], c["down"], P["M"])
    tr = mse.RaterTrainer(rater, lr=P["lr"])
    losses = tr.run(c["rows"], c["pair_ids"], c["targets"])
    assert losses.shape == (P["steps"],) and tr.steps == P["steps"]
    assert_same(device_snapshot(rater, tr), snapshot(model), "after %d steps" % P["steps"])
    # the held-out figures from the device's own member scores
    held = c["held"].astype(np.int64)
    s = rater.member_scores(c["rows"]).to_host()[:, :, 0]
    z = s[held[:, 0]] - s[held[:, 1]]
    assert float(((z.astype(np.float64).mean(axis=1) > 0) == (c["held_ratings"][:, 0] > 0.5)).mean()) == after[1]
