"""Thresholded group maxima of the 320-query pass (bruteforce.hip mfma_pass): every S-th 256-row tile is scanned first and gives
each query a threshold tau; the scan of the other tiles keeps a group maximum only above tau, in a per-query list.  The answers must be
what the dense array of maxima gives: every case runs the search forced-sparse, forced-off and in the exact mode and wants equal ids and
i64 scores, and the oracle's where it is computed (all of these bases are small enough).
Shapes: S = 3 and 5 over (2 S + 1) tiles -- the last tile then IS a sample tile -- plus tails of 1 .. 255 rows, whose tile is not; 257
queries (zero-padded columns) and 320; k = 1, 10, 100; a non-zero id offset; random rows, a sorted base (the best rows in a tile the
sample does not see), 40 exact copies of the best row (ties above tau, widening until the list is used up), all rows equal and a list
capacity of 8 (overflow: the dense fallback, counted), k above the sample's group count (dense by itself), two shards on one device."""
import functools

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152


@functools.lru_cache(maxsize=None)
def _rows(seed, stream, n):
    from oracle import orc
    a = orc.gen_rows_f16(seed, stream, n)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle_random(n, nq, k):
    from oracle import orc
    return orc.bruteforce_topk(_rows(SEED_BASE, 41, n), _rows(SEED_QUERY, 41, 320)[:nq], k)


def three_ways(mse, base, q, k, stride, want=None, capacity=8192, sparse_expected=True, fallback_expected=False):
    """forced-sparse == forced-off == exact (== the oracle's answer `want`); returns the searcher's statistics of the forced-sparse call"""
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    s.set_sparse_maxima("forced", stride, capacity)
    ss, si = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    st = s.last_stats()
    print("forced sparse:", st)
    s.set_sparse_maxima("off")
    ds, di = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert s.last_stats()["sparse_passes"] == 0
    es, ei = s.bruteforce_topk(q, k, mse.MODE_EXACT)
    assert np.array_equal(si, di) and np.array_equal(ss, ds), "sparse differs from dense"
    assert np.array_equal(si, ei) and np.array_equal(ss, es), "sparse differs from the exact mode"
    if want is not None:
        assert np.array_equal(si, want[1]) and np.array_equal(ss, want[0]), "sparse differs from the oracle"
    assert st["sparse_passes"] == (1 if sparse_expected else 0), st
    assert st["sparse_fallbacks"] == (1 if fallback_expected else 0), st
    s.close()
    return st


# (2 S + 1) tiles: tiles 0, S and 2 S are the sample, the last tile among them; a tail adds a tile that is not
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("tail", [0, 1, 63, 65, 255])
@pytest.mark.parametrize("stride", [3, 5])
def test_sizes_and_tails(gpu, mse, orc, stride, tail, nq):
    n = (2 * stride + 1) * 256 + tail
    three_ways(mse, _rows(SEED_BASE, 41, n), _rows(SEED_QUERY, 41, 320)[:nq], 10, stride, _oracle_random(n, nq, 10))


# 80 tiles and a ragged one: 27 sample tiles = 108 sample groups, enough for k = 100; the ids carry an offset past 2^31
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_k_and_id_offset(gpu, mse, orc, k, nq):
    import torch
    n, off = 80 * 256 + 65, (1 << 31) + 12345
    base, q = _rows(SEED_BASE, 41, n), _rows(SEED_QUERY, 41, 320)[:nq]
    ws, wi = _oracle_random(n, nq, k)
    three_ways(mse, base, q, k, 3, (ws, wi))
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    s.set_sparse_maxima("forced", 3)
    qd = torch.from_numpy(q.view(np.int16).copy()).cuda()
    out_s = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    out_i = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    s.bruteforce_topk_dev(qd.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA, id_offset=off)
    torch.cuda.synchronize()
    assert s.last_stats()["sparse_passes"] == 1
    assert np.array_equal(out_i.cpu().numpy().view(np.uint32), (wi.astype(np.uint64) + off).astype(np.uint32))
    assert np.array_equal(out_s.cpu().numpy(), ws)
    s.close()


def _clustered_queries(orc, nq, seed):
    """queries around one direction, so that one ordering of the rows is 'sorted' for all of them"""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal(D)
    proto /= np.linalg.norm(proto)
    qf = proto + 0.3 * rng.standard_normal((nq, D)) / np.sqrt(D)
    return proto, orc.f16_bits((qf / np.linalg.norm(qf, axis=1, keepdims=True)).astype(np.float32))


# rows ascending by their score against the queries' common direction: the best 255 rows lie in the last tile, which the sample does
# not see, so tau sits below the true k-th score and the lists hold every group of that tile and more
@pytest.mark.parametrize("nq", [257, 320])
def test_sorted_base(gpu, mse, orc, nq):
    stride = 5
    n = (2 * stride + 1) * 256 + 255
    proto, q = _clustered_queries(orc, nq, 43)
    base = _rows(SEED_BASE, 43, n)
    base = base[np.argsort(orc.f16_to_f32(base).astype(np.float64) @ proto, kind="stable")]
    st = three_ways(mse, np.ascontiguousarray(base), q, 10, stride, orc.bruteforce_topk(base, q, 10))
    assert st["sparse_longest_list"] >= 4   # at least the last tile's four groups hold rows above every sample row


# 40 exact copies of the row every query likes best, one per tile of tiles 0 .. 39 (14 of them sample tiles at S = 3): the ten best
# are tied copies, the first round's 18th group key equals the k-th score, and the widening takes the list until it is used up
@pytest.mark.parametrize("nq", [257, 320])
def test_forty_copies_in_distinct_groups(gpu, mse, orc, nq):
    n = 44 * 256 + 65
    proto, q = _clustered_queries(orc, nq, 47)
    base = _rows(SEED_BASE, 47, n).copy()
    rng = np.random.default_rng(47)
    at = np.arange(40) * 256 + rng.integers(0, 256, 40)
    base[at] = orc.f16_bits(proto.astype(np.float32))
    ws, wi = orc.bruteforce_topk(base, q, 10)
    assert np.isin(wi, at).all()   # the case is what it says: every answer row is a copy
    st = three_ways(mse, base, q, 10, 3, (ws, wi))
    assert st["widened_queries"] > 0 and st["max_groups"] > 18, st


# all rows equal: every group's maximum is above tau, all 29 of them; with room for 16 the lists overflow and the dense path answers
@pytest.mark.parametrize("nq", [257, 320])
def test_all_rows_equal_overflows(gpu, mse, orc, nq):
    n = 7 * 256 + 65
    base = np.ascontiguousarray(np.tile(_rows(SEED_BASE, 53, 1), (n, 1)))
    q = _rows(SEED_QUERY, 53, 320)[:nq]
    st = three_ways(mse, base, q, 10, 3, orc.bruteforce_topk(base, q, 10), capacity=16, fallback_expected=True)
    assert st["sparse_longest_list"] == (n + 63) // 64


# random rows and room for 8 survivors where about k * S are expected: the fallback is counted, the answers stand
@pytest.mark.parametrize("nq", [257, 320])
def test_capacity_of_eight(gpu, mse, orc, nq):
    n = 80 * 256 + 65
    st = three_ways(mse, _rows(SEED_BASE, 41, n), _rows(SEED_QUERY, 41, 320)[:nq], 10, 3, _oracle_random(n, nq, 10), capacity=8,
                    fallback_expected=True)
    assert st["sparse_longest_list"] > 8


# 12 sample groups and k = 50: no k-th sample maximum exists, the forced call takes the dense path by itself; and the automatic mode
# leaves a base this small alone
def test_k_above_the_sample_and_auto_on_a_small_base(gpu, mse, orc):
    n, nq = 7 * 256 + 65, 320
    base, q = _rows(SEED_BASE, 41, n), _rows(SEED_QUERY, 41, 320)
    three_ways(mse, base, q, 50, 3, _oracle_random(n, nq, 50), sparse_expected=False)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    ws, wi = _oracle_random(n, nq, 10)
    gs, gi = s.bruteforce_topk(q, 10, mse.MODE_MFMA)
    assert s.last_stats()["sparse_passes"] == 0
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws)
    s.close()


def test_two_shards_on_one_device(gpu, mse, orc):
    n, nq, k = 9000 + 41, 320, 10
    q = _rows(SEED_QUERY, 59, nq)
    ws, wi = orc.bruteforce_topk(orc.gen_rows_f16(SEED_BASE, 0, n), q, k)
    whole = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    whole.set_sparse_maxima("off")
    us, ui = whole.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert np.array_equal(ui, wi) and np.array_equal(us, ws)
    grp = mse.ShardGroup(2, D, devices=[0, 0])
    grp.generate(SEED_BASE, 0, n)
    for g in range(2):
        grp.searcher(g).set_sparse_maxima("forced", 3)
    s, i = grp.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert np.array_equal(i, ui) and np.array_equal(s, us)
    stats = [grp.searcher(g).last_stats() for g in range(2)]
    assert all(st["sparse_passes"] == 1 and st["sparse_fallbacks"] == 0 for st in stats), stats
    grp.close()
    whole.close()
