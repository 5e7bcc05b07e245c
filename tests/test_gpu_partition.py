"""The shard partition on the device (include/mse.h mse_partitioner) against its numpy restatement tests/partition_ref.py.
Every comparison is for equality: the header defines the results on f64 values the device has to reproduce bit for bit."""
import functools

import numpy as np
import pytest

import partition_ref as ref
from conftest import SEED_BASE, SEED_CENTRES, SEED_QUERY

pytestmark = pytest.mark.gpu

SHAPES = [(n, S, d) for d in (1152, 40) for S in (2, 6, 42, 64) for n in (6, 1000, 2048) if n >= S]


@functools.lru_cache(maxsize=None)
def rows_of(n, d):
    from oracle import orc
    orc.build()
    return ref.skewed_rows(orc, n, SEED_BASE, SEED_CENTRES, d)


@functools.lru_cache(maxsize=None)
def centroids_of(S, d, duplicate=True):
    """normalised noise; the last centroid repeats the first (S >= 3), so every row has a tie the rule has to break"""
    from oracle import orc
    c = ref.normalise(np.stack([ref.noise(orc, 77, 1000 + s, d) for s in range(S)]))
    if duplicate and S >= 3:
        c[S - 1] = c[0]
    return c


@functools.lru_cache(maxsize=None)
def pass_reference(n, S, d):
    sc = ref.scores(rows_of(n, d), centroids_of(S, d))
    t2 = ref.top2(sc)
    return sc, t2, ref.sizes_of(t2, S)


@pytest.mark.parametrize("n,S,d", SHAPES)
def test_counting_pass_and_scores_out(gpu, mse, n, S, d):
    sc, t2, sizes = pass_reference(n, S, d)
    if S >= 3:
        assert np.all(t2[:, 0] != S - 1) and np.all(t2[t2[:, 1] == S - 1, 0] == 0)   # the duplicate loses every tie to centroid 0
        assert np.any(t2[:, 1] == S - 1) or n < 100
    p = mse.ShardPartitioner(S, d).set_sample(rows_of(n, d))
    got_sizes, got_t2 = p.count(centroids_of(S, d), top2=True)
    assert np.array_equal(got_t2, t2)
    assert np.array_equal(got_sizes, sizes)
    if S == 2:
        assert np.all(got_sizes.sum(axis=0) == n)                                  # every row is in both ranks: best of one shard, second of the other
    assert p.scores(centroids_of(S, d)).tobytes() == sc.tobytes()
    p.close()


@pytest.mark.parametrize("n,S,d", [(1000, 6, 1152), (2048, 42, 1152), (1000, 64, 1152)])   # (a base is a multiple of 64 wide)
def test_pass_over_a_base_with_a_shuffled_id_list_and_in_row_chunks(gpu, mse, n, S, d):
    sc, t2, sizes = pass_reference(n, S, d)
    rows = rows_of(n, d)
    perm = np.random.default_rng(n + S).permutation(n).astype(np.uint32)
    shuffled = np.ascontiguousarray(rows[np.argsort(perm)])            # base row perm[i] = sample row i
    base = mse.VectorList.from_f16s(shuffled, d)
    p = mse.ShardPartitioner(S, d).set_sample(base, perm)
    got_sizes, got_t2 = p.count(centroids_of(S, d), top2=True)
    assert np.array_equal(got_t2, t2) and np.array_equal(got_sizes, sizes)
    from mse import ffi
    ffi.check(ffi.lib().mse_debug_partition_chunk_rows(p._h, 300))     # a ragged last chunk of the scores-out form
    assert p.scores(centroids_of(S, d)).tobytes() == sc.tobytes()
    p.close()


def test_noise_and_normalisation(gpu, mse, orc):
    from mse import ffi
    L = ffi.lib()
    for seed, key, d in [(3, 0, 1152), (3, 5, 1152), (9, (1 << 40) + 7 * 6 + 2, 1152), (1, 11, 40)]:
        out = np.empty(d, np.float32)
        ffi.check(L.mse_debug_partition_noise(seed, key, d, out.ctypes.data_as(ffi.f32p)))
        assert out.tobytes() == (orc.gen_row_ints(seed, key, d).astype(np.float32) * ref.K).tobytes()
    c = np.stack([ref.noise(orc, 5, s, 1152) for s in range(5)])
    c[1] *= np.float32(1e-12)
    c[2] *= np.float32(3e7)
    c[3] = 0.0
    out, h = np.empty_like(c), np.empty(c.shape, np.uint16)
    ffi.check(L.mse_debug_partition_normalise(c.ctypes.data_as(ffi.f32p), 5, 1152, out.ctypes.data_as(ffi.f32p), h.ctypes.data_as(ffi.u16p)))
    want = ref.normalise(c)
    assert out.tobytes() == want.tobytes()
    assert not out[3].any()                                             # a zero row stays zero
    assert np.array_equal(h, want.astype(np.float16).view(np.uint16))
    assert np.all(np.abs(np.linalg.norm(want[[0, 1, 2, 4]].astype(np.float64), axis=1) - 1.0) < 1e-6)


ANNEAL = dict(reroll_after=3, stop_fraction=0.0, seed=3)


@pytest.fixture(scope="module")
def annealed(orc):
    return ref.Annealer(orc, rows_of(2048, 1152), 6, **ANNEAL).run(64)


def run_device(mse, calls, **config):
    p = mse.ShardPartitioner(6, 1152, **config).set_sample(rows_of(2048, 1152))
    F, code = [], []
    for iters in calls:
        f, c = p.anneal(iters)
        F.append(f)
        code.append(c)
    return p, np.concatenate(F), np.concatenate(code)


def test_annealing_equals_the_restatement(gpu, mse, annealed):
    want_F = np.array([f for f, _ in annealed.trace], np.uint64)
    want_code = np.array([c for _, c in annealed.trace], np.uint8)
    assert set(want_code.tolist()) == {0, 1, 2}                          # every branch of the loop is taken
    p, F, code = run_device(mse, [64], **ANNEAL)
    assert np.array_equal(F, want_F) and np.array_equal(code, want_code)
    st = p.state()
    assert (st.t, st.last_fitness, st.last_improvement, st.stopped) == (64, annealed.last, annealed.li, 0)
    assert np.float32(st.temperature).tobytes() == np.float32(annealed.T).tobytes()
    raw, nrm, h = p.raw_centroids(), p.centroids(), p.centroids_f16()
    assert raw.tobytes() == annealed.c.tobytes()
    assert nrm.tobytes() == ref.normalise(annealed.c).tobytes()
    assert np.array_equal(h, ref.normalise(annealed.c).astype(np.float16).view(np.uint16))
    # a second run gives the same bytes; 64 iterations in one call equal 2 x 32
    p2, F2, code2 = run_device(mse, [64], **ANNEAL)
    assert np.array_equal(F2, F) and np.array_equal(code2, code) and p2.raw_centroids().tobytes() == raw.tobytes()
    p3, F3, code3 = run_device(mse, [32, 32], **ANNEAL)
    assert np.array_equal(F3, F) and np.array_equal(code3, code) and p3.raw_centroids().tobytes() == raw.tobytes()
    assert p3.centroids().tobytes() == nrm.tobytes() and np.float32(p3.state().temperature) == np.float32(st.temperature)


def test_annealing_stops_where_the_restatement_stops(gpu, mse, orc):
    cfg = dict(ANNEAL, stop_fraction=0.5)
    want = ref.Annealer(orc, rows_of(2048, 1152), 6, **cfg).run(64)
    assert want.stopped and 1 <= want.t < 64
    p, F, code = run_device(mse, [64], **cfg)
    st = p.state()
    assert st.stopped == 1 and st.t == want.t and len(F) == want.t
    assert np.array_equal(F, np.array([f for f, _ in want.trace], np.uint64))
    assert np.float32(st.temperature).tobytes() == np.float32(want.T).tobytes()
    raw = p.raw_centroids()
    assert raw.tobytes() == want.c.tobytes()
    f, c = p.anneal(16)                                                   # later calls change nothing
    assert len(f) == 0 and p.state().t == want.t and p.raw_centroids().tobytes() == raw.tobytes()


@functools.lru_cache(maxsize=None)
def assign_case(n, S, duplicate=False):
    c16 = centroids_of(S, 1152, duplicate).astype(np.float16).view(np.uint16)
    return c16, ref.scores(rows_of(n, 1152), ref.widen(c16))


@pytest.mark.parametrize("n,S", [(1000, 6), (2048, 6), (1000, 42), (2048, 42)])
def test_assignment_equals_the_restatement(gpu, mse, n, S):
    c16, sc = assign_case(n, S)
    pairs = {}
    for fudge in (0.2, 0.0):
        want, want_counts, _ = ref.walk(sc, fudge)
        p = mse.ShardPartitioner(S).set_centroids(c16).assign(rows_of(n, 1152), fudge)
        assert np.array_equal(p.assignment(), want)
        assert np.array_equal(p.counts(), want_counts.astype(np.uint64)) and int(p.counts().sum()) == 2 * n
        pairs[fudge] = want
        p.close()
    assert np.any(np.sort(pairs[0.2], axis=1) != np.sort(pairs[0.0], axis=1))   # the fudge changes some row's pair


def test_assignment_streamed_chunked_tied_and_with_an_extreme_fudge(gpu, mse):
    from mse import ffi
    n, S = 1000, 6
    rows = rows_of(n, 1152)
    c16, sc = assign_case(n, S)
    want, want_counts, _ = ref.walk(sc, 0.2)
    p = mse.ShardPartitioner(S).set_centroids(c16)
    for r0 in range(0, n, 300):                                           # streamed: counts and bal carry on
        p.assign(rows[r0:r0 + 300], 0.2)
    assert np.array_equal(p.assignment(), want) and np.array_equal(p.counts(), want_counts.astype(np.uint64))
    p.reset_assignment()
    ffi.check(ffi.lib().mse_debug_partition_chunk_rows(p._h, 256))        # four score chunks in flight against the walk
    base = mse.VectorList.from_f16s(rows, 1152)
    p.assign(base, 0.2)
    assert np.array_equal(p.assignment(), want) and p.n_assigned() == n
    # duplicate centroids: the keys of shards 0 and S - 1 are equal while their counts are, and the lowest index wins
    d16, dsc = assign_case(n, S, True)
    dwant, dcounts, _ = ref.walk(dsc, 0.0)
    assert np.all(dwant[np.any(dwant == S - 1, axis=1)] == [0, S - 1])
    p.reset_assignment().set_centroids(d16).assign(rows, 0.0)
    assert np.array_equal(p.assignment(), dwant) and np.array_equal(p.counts(), dcounts.astype(np.uint64))
    # an extreme fudge: the balance term rules.  A shard that leads another by more than R bal / fudge rows (R: the spread of the scores)
    # loses to it whatever the scores, so the counts stay that close: a near round robin
    xwant, xcounts, _ = ref.walk(sc, 5.0)
    assert xcounts.max() - xcounts.min() <= (sc.max() - sc.min()) * (n + 1) / 5.0 + 2
    p.reset_assignment().set_centroids(c16).assign(rows, 5.0)
    assert np.array_equal(p.assignment(), xwant) and np.array_equal(p.counts(), xcounts.astype(np.uint64))


def test_shard_filters_members_and_a_filtered_search(gpu, mse, orc):
    n, S = 1000, 6
    rows = rows_of(n, 1152)
    c16, _ = assign_case(n, S)
    base = mse.VectorList.from_f16s(rows, 1152)
    p = mse.ShardPartitioner(S).set_centroids(c16).assign(base, 0.2)
    a = p.assignment()
    assert int(p.counts().sum()) == 2 * n
    for s in range(S):
        f = p.shard_filter(s)
        mask = np.any(a == s, axis=1)
        assert len(f) == n and np.array_equal(f.to_mask(), mask)
        m = p.members(s)
        assert np.array_equal(m, np.flatnonzero(mask).astype(np.uint32)) and m.size == int(p.counts()[s])
        f.close()
    s = int(np.argmax(p.counts()))
    f, m = p.shard_filter(s), p.members(s)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 4)
    got_s, got_i = mse.Searcher(base).bruteforce_topk(q, 10, mse.MODE_EXACT, allow=f)
    want_s, want_i = orc.bruteforce_topk(rows[m], q, 10)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_i, m[want_i])


def test_medioid_ids_and_entries(gpu, mse, orc):
    n, S = 1000, 6
    rows = rows_of(n, 1152)
    base = mse.VectorList.from_f16s(rows, 1152)
    rng = np.random.default_rng(5)
    for ids in (rng.permutation(n)[:400], np.array([123]), rng.integers(0, 50, 200)):
        ids = ids.astype(np.uint32)
        assert mse.medioid_ids(base, ids) == orc.medioid(rows[ids])
    c16, _ = assign_case(n, S)
    p = mse.ShardPartitioner(S).set_centroids(c16).assign(base, 0.2)
    cen, node_ids = p.entries(base)
    members = [p.members(s) for s in range(S)]
    by_hand = np.array([m[orc.medioid(rows[m])] for m in members], np.uint32)
    assert cen.tobytes() == ref.widen(c16).tobytes() and np.array_equal(node_ids, by_hand)
    g = mse.BuildGraph(n, 16)
    g.random_fill(7)
    s = mse.Searcher(base)
    q = orc.f16_to_f32(orc.gen_rows_f16(SEED_QUERY, 0, 3))
    mse.set_entry_centroids(g, cen, node_ids)
    got = mse.disk_query_topk(s, None, None, g, q, 5, None, None, None, True, 2, 16)
    mse.set_entry_centroids(g, ref.widen(c16), by_hand)
    want = mse.disk_query_topk(s, None, None, g, q, 5, None, None, None, True, 2, 16)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    starts = [int(by_hand[orc.select_shard(ref.widen(c16), q[i])]) for i in range(3)]
    assert all(0 <= x < n for x in starts)
