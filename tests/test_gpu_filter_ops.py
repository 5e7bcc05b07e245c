"""Row filters as values on the device: set algebra (mse_filter_combine / _not), the descriptor predicate (mse_filter_from_descriptors),
the score threshold (mse_filter_from_scores), device bits in (mse_filter_from_bits_dev) and the read-back (mse_filter_to_bits /
_read_ids).  Every expected value is numpy on boolean masks or the CPU oracle's score_all, every assertion an equality.  A new filter's
mask, count and ids are checked BEFORE any search consumes it: a stray bit past n_rows is then a failed assert, not an out-of-range read."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY, make_pq
from test_gpu_filtered_graph import clustered_rows, knn_graph
from test_gpu_graph_delete import cfgs

pytestmark = pytest.mark.gpu
D = 1152
NONE = 0xFFFFFFFF
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
# word (32) and tile (256) boundaries, the compaction block (8192 rows), and several blocks with a ragged end
SIZES = [1, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193, 70_001]


def check(f, want, tag=None):
    """f is exactly the boolean mask `want`: length, bitmap, count and ascending id list"""
    want = np.asarray(want, bool)
    assert len(f) == want.size, tag
    got = f.to_mask()
    assert got.dtype == np.bool_ and got.shape == want.shape and np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:5])
    assert f.count == int(want.sum()), tag
    ids = f.ids()
    assert ids.dtype == np.uint32 and np.array_equal(ids, np.flatnonzero(want)), tag


def densities(n, rng):
    one = np.zeros(n, bool)
    one[rng.integers(n)] = True
    return {"none": np.zeros(n, bool), "one bit": one, "50 %": rng.random(n) < 0.5, "all": np.ones(n, bool)}


OPS = {"&": (lambda a, b: a & b, lambda a, b: a & b), "|": (lambda a, b: a | b, lambda a, b: a | b),
       "^": (lambda a, b: a ^ b, lambda a, b: a ^ b), "-": (lambda a, b: a - b, lambda a, b: a & ~b)}


# ---- 1. algebra against numpy ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_algebra_matches_numpy(gpu, mse, n):
    """The four ops and ~ on every pair of densities none / one bit / 50 % / all; the operands read back unchanged afterwards."""
    rng = np.random.default_rng(n)
    ma, mb = densities(n, rng), densities(n, rng)
    fa = {k: mse.RowFilter(m) for k, m in ma.items()}
    fb = {k: mse.RowFilter(m) for k, m in mb.items()}
    for ka, a in ma.items():
        r = ~fa[ka]
        check(r, ~a, ("~", ka))
        r.close()
        for kb, b in mb.items():
            for name, (dev_op, np_op) in OPS.items():
                r = dev_op(fa[ka], fb[kb])
                check(r, np_op(a, b), (name, ka, kb))
                r.close()
    for k in ma:
        check(fa[k], ma[k], ("operand a", k))
        check(fb[k], mb[k], ("operand b", k))
        fa[k].close()
        fb[k].close()


def test_algebra_operands_of_different_lengths(gpu, mse):
    """257 against 8193 rows, both ways round: the result has the longer length and the short operand reads as zeros past its end."""
    rng = np.random.default_rng(1)
    s, l = rng.random(257) < 0.5, rng.random(8193) < 0.5
    padded = np.zeros(8193, bool)
    padded[:257] = s
    fs, fl = mse.RowFilter(s), mse.RowFilter(l)
    for name, (dev_op, np_op) in OPS.items():
        check(dev_op(fs, fl), np_op(padded, l), (name, "short first"))
        check(dev_op(fl, fs), np_op(l, padded), (name, "long first"))
    # all-ones operands: a kernel that read the short operand past its end, or padded it with ones, shows here
    ones_s, ones_l = mse.RowFilter(np.ones(257, bool)), mse.RowFilter(np.ones(8193, bool))
    check(ones_s & ones_l, np.arange(8193) < 257, "ones & ones")
    check(ones_l - ones_s, np.arange(8193) >= 257, "ones - ones")
    check(ones_s - ones_l, np.zeros(8193, bool), "short ones - long ones")
    check(fs, s, "short operand unchanged")
    check(fl, l, "long operand unchanged")


def test_invert_lengths_and_lifetimes(gpu, mse, orc):
    rng = np.random.default_rng(2)
    m = rng.random(257) < 0.5
    f = mse.RowFilter(m)
    for n_rows in (257, 258, 288, 512, 513, 8193):                          # the new rows come out allowed
        want = np.ones(n_rows, bool)
        want[:257] = ~m
        check(f.invert(n_rows), want, n_rows)
    check(~mse.RowFilter(np.ones(33, bool)), np.zeros(33, bool), "~ all ones over 33 rows")
    assert (~mse.RowFilter(np.ones(33, bool))).count == 0
    # ~ of an empty filter over 257 rows allows exactly 257 rows, and a search under it returns them all and then padding
    full = ~mse.RowFilter(np.zeros(257, bool))
    check(full, np.ones(257, bool), "~ none over 257 rows")
    base = orc.gen_rows_f16(SEED_BASE, 0, 257)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 1)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    sc, ids = s.bruteforce_topk(q, 300, mse.MODE_EXACT, allow=full)
    ws, wi = orc.bruteforce_topk(base, q, 257)
    assert np.array_equal(ids[0, :257], wi[0]) and np.array_equal(sc[0, :257], ws[0])
    assert (ids[0, 257:] == NONE).all() and (sc[0, 257:] == I64_MIN).all()
    # a result outlives its operands
    a, b = rng.random(8193) < 0.5, rng.random(8193) < 0.5
    fa, fb = mse.RowFilter(a), mse.RowFilter(b)
    r = fa ^ fb
    fa.close()
    fb.close()
    junk = [mse.RowFilter(np.ones(8193, bool)) for _ in range(4)]            # allocations that may land where the operands were
    check(r, a ^ b, "after both operands are closed")
    check(~r, ~(a ^ b))
    del junk


# ---- 2. descriptor predicate against numpy --------------------------------------------------------------------------------------

def desc_ranges(n_desc, rng):
    bands = {j: tuple(sorted(int(v) for v in rng.integers(0, 256, 2))) for j in range(n_desc)}
    return {"full": {}, "a single value": {0: (7, 7)}, "a band on one channel": {n_desc - 1: (64, 191)}, "bands on all channels": bands,
            "lo > hi": {0: (200, 100)}, "edges": {0: (0, 0), n_desc - 1: (255, 255)}}


def desc_mask(desc, ranges):
    m = np.ones(desc.shape[0], bool)
    for j, (lo, hi) in ranges.items():
        m &= (desc[:, j] >= lo) & (desc[:, j] <= hi)
    return m


@pytest.mark.parametrize("n_desc", [4, 1, 3])
def test_descriptor_predicate_matches_numpy(gpu, mse, n_desc):
    for n in SIZES:
        rng = np.random.default_rng(n * 8 + n_desc)
        desc = rng.integers(0, 256, size=(n, n_desc), dtype=np.uint8)
        desc[rng.random(n) < 0.3, 0] = 7                                    # "a single value" selects something
        edge = rng.random(n) < 0.1                                          # "edges" selects something
        desc[edge, 0], desc[edge, n_desc - 1] = 0, 255
        codes = mse.Codes(rng.integers(0, 256, size=(n, 8), dtype=np.uint8), desc)
        for name, ranges in desc_ranges(n_desc, rng).items():
            if name == "edges" and n_desc == 1:
                continue                                                     # one channel cannot be 0 and 255
            want = desc_mask(desc, ranges)
            f = mse.RowFilter.from_descriptors(codes, ranges)
            check(f, want, (n, name))
            f.close()
        codes.close()


def test_descriptor_argument_checks(gpu, mse):
    codes = mse.Codes(np.zeros((5, 8), np.uint8), np.zeros((5, 3), np.uint8))
    for bad in ({3: (0, 1)}, {-1: (0, 1)}, {0: (0, 256)}, {0: (-1, 5)}):
        with pytest.raises(ValueError):
            mse.RowFilter.from_descriptors(codes, bad)


# ---- the 3 000-row index with codes, descriptors and a graph ----------------------------------------------------------------------

class Index3k:
    N, R, K = 3000, 150, 10

    def __init__(self, mse, orc):
        n = self.N
        rng = np.random.default_rng(404)
        self.rng = rng
        self.x = clustered_rows(orc, n, D, n_centres=20, seed=405)
        self.rows = orc.f16_bits(self.x)
        cents, T, dpc, _ = make_pq(orc, D, D // 64)
        self.opq, self.gpq = orc.PQ(cents, T, dpc, D), mse.ProductQuantizer(cents, T, dpc, D)
        self.codes = self.opq.quantize_batch(orc.f16_to_f32(self.rows))
        self.desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
        self.scales = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)
        self.adj, self.deg = knn_graph(self.x, 16, rng)
        self.has_url = (rng.random(n) > 0.2).astype(np.uint8)
        self.entry = 1500
        self.has_url[self.entry] = 1
        self.vecs = mse.VectorList.from_f16s(self.rows, D)
        self.searcher = mse.Searcher(self.vecs)
        self.gcodes = mse.Codes(self.codes, self.desc)
        _, self.mcfg = cfgs(orc, mse, r=16, l=64, maxc=250)
        self.mse = mse
        self.qs = clustered_rows(orc, 6, D, n_centres=20, seed=406)
        self.qh = orc.f16_bits(self.qs)

    def graph(self):
        return self.mse.DeviceGraph(self.mse.IndexGraph(self.adj, self.deg), self.has_url)


@pytest.fixture(scope="module")
def deleted_index(gpu, mse, orc):
    """the index with a third of its rows deleted (never the entry node); nothing in this module changes it afterwards"""
    ix = Index3k(mse, orc)
    ix.g = ix.graph()
    ix.dead = np.zeros(ix.N, bool)
    ix.dead[ix.rng.choice(np.setdiff1d(np.arange(ix.N), [ix.entry]), ix.N // 3, replace=False)] = True
    assert ix.g.delete_rows(ix.searcher, np.flatnonzero(ix.dead), ix.mcfg)["deleted"] == ix.N // 3
    return ix


def test_descriptor_predicate_sees_inserted_rows(gpu, mse, orc):
    """insert_rows writes new descriptor bytes into freed slots: a filter made afterwards is about the new bytes, one made before is not."""
    ix = Index3k(mse, orc)
    g = ix.graph()
    slots = np.sort(ix.rng.choice(np.setdiff1d(np.arange(ix.N), [ix.entry]), 200, replace=False)).astype(np.uint32)
    assert g.delete_rows(ix.searcher, slots, ix.mcfg)["deleted"] == 200
    ranges = {1: (0, 99), 2: (50, 255)}
    before = mse.RowFilter.from_descriptors(ix.gcodes, ranges)
    check(before, desc_mask(ix.desc, ranges), "before the insert")
    new_desc = np.empty((200, 4), np.uint8)
    new_desc[:] = 255 - ix.desc[slots]                                       # every new row differs from the one it replaces
    new_rows = orc.f16_bits(clustered_rows(orc, 200, D, n_centres=20, seed=407))
    assert g.insert_rows(ix.searcher, slots, new_rows, ix.mcfg, ix.entry, ix.gpq, ix.gcodes, new_desc)["inserted"] == 200
    desc_now = ix.desc.copy()
    desc_now[slots] = new_desc
    assert np.array_equal(ix.gcodes.read_rows(0, ix.N, descriptors=True)[1], desc_now)
    after = mse.RowFilter.from_descriptors(ix.gcodes, ranges)
    want = desc_mask(desc_now, ranges)
    assert not np.array_equal(want, desc_mask(ix.desc, ranges))
    check(after, want, "after the insert")
    check(before, desc_mask(ix.desc, ranges), "the old filter is a value")
    g.close()


# ---- 3. score threshold against the oracle --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d", [(1, D), (257, D), (8193, D), (257, 192)])
def test_score_threshold_matches_oracle(gpu, mse, orc, n, d):
    rng = np.random.default_rng(n + d)
    base = orc.gen_rows_f16(SEED_BASE, 0, n, d)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 1, d)[0]
    kth = min(10, n)
    tenth = int(orc.bruteforce_topk(base, q, kth)[1][0, kth - 1])
    twin = None
    if n > 20:                                                               # the base holds the 10th-best row twice
        twin = int(np.setdiff1d(np.arange(n), orc.bruteforce_topk(base, q, 12)[1][0])[n // 2])
        base[twin] = base[tenth]
    scores = orc.score_all(base, q)
    t = int(scores[tenth])
    s = mse.Searcher(mse.VectorList.from_f16s(base, d))
    assert np.array_equal(s.scores(q), scores)
    half = rng.random(n) < 0.5
    within = mse.RowFilter(half)
    for name, thr in (("INT64_MIN", I64_MIN), ("INT64_MAX", I64_MAX), ("10th best", t), ("10th best + 1", t + 1)):
        want = np.array([int(v) >= thr for v in scores], bool)
        f = mse.RowFilter.from_scores(s, q, thr)
        check(f, want, (name, "all rows"))
        if name == "INT64_MIN":
            assert f.count == n
        if name == "INT64_MAX":
            assert f.count == int((scores == I64_MAX).sum())
        if twin is not None and name == "10th best":
            assert want[tenth] and want[twin]                               # >= : both copies are in
        if twin is not None and name == "10th best + 1":
            assert not want[tenth] and not want[twin] and f.count > 0       # both copies are out, the better rows stay
        fw = mse.RowFilter.from_scores(s, q, thr, within=within)
        check(fw, want & half, (name, "within 50 %"))
        check(f & within, want & half, (name, "the AND"))
        f.close()
        fw.close()
    check(within, half, "within unchanged")
    if n > 40:                                                               # a `within` shorter than the base: zeros past its end
        short = mse.RowFilter(half[:n - 37])
        want = scores >= t
        want[n - 37:] = False
        check(mse.RowFilter.from_scores(s, q, t, within=short), want & np.concatenate([half[:n - 37], np.zeros(37, bool)]), "short within")


def test_range_search_over_the_live_rows(deleted_index, mse, orc):
    """within=live_filter() on an index after a delete: ids() is the sorted oracle answer over the live rows."""
    ix = deleted_index
    live = ix.g.live_filter()
    check(live, ~ix.dead, "live filter")
    for j in range(3):
        scores = orc.score_all(ix.rows, ix.qh[j])
        thr = int(np.sort(scores)[-60])                                      # some sixty rows reach it, some of them deleted
        f = mse.RowFilter.from_scores(ix.searcher, ix.qh[j], thr, within=live)
        want = (scores >= thr) & ~ix.dead
        assert 0 < want.sum() < (scores >= thr).sum()
        check(f, want, j)
        assert np.array_equal(f.ids(), np.flatnonzero(want).astype(np.uint32))
        f.close()


# ---- 4. consumers cannot tell a filter built on the device from one built from a numpy mask ----------------------------------------

def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_consumers_cannot_tell(deleted_index, mse, orc):
    ix = deleted_index
    ranges = {0: (64, 255), 3: (0, 200)}
    mask = desc_mask(ix.desc, ranges) & ~ix.dead
    dev = mse.RowFilter.from_descriptors(ix.gcodes, ranges) & ix.g.live_filter()
    check(dev, mask, "from_descriptors & live_filter")
    host = mse.RowFilter(mask)
    assert 10 * ix.K < dev.count < ix.N // 2
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA):
        a, b = ix.searcher.bruteforce_topk(ix.qh, ix.K, mode, allow=dev), ix.searcher.bruteforce_topk(ix.qh, ix.K, mode, allow=host)
        assert same(a, b) and (a[1] != NONE).all() and mask[a[1]].all(), mode
    for mode in ("scan", "list"):
        for s in (None, ix.searcher):
            a = ix.gpq.scan_topk_batch_filtered(ix.gcodes, dev, ix.qs, ix.R, ix.K, s, ix.scales, mode)
            b = ix.gpq.scan_topk_batch_filtered(ix.gcodes, host, ix.qs, ix.R, ix.K, s, ix.scales, mode)
            assert same(a, b) and mask[a[1]].all(), (mode, s is not None)
    starts = np.full(6, ix.entry, np.uint32)
    for regime in ("graph", "list"):
        a = mse.disk_query_topk(ix.searcher, None, ix.gcodes, ix.g, ix.qh, ix.K, starts, None, ix.scales, True, 4, 64, filter=dev, regime=regime)
        b = mse.disk_query_topk(ix.searcher, None, ix.gcodes, ix.g, ix.qh, ix.K, starts, None, ix.scales, True, 4, 64, filter=host, regime=regime)
        assert same(a[:2], b[:2]), regime
        got = a[0][a[0] != NONE]
        assert got.size and mask[got].all() and (ix.has_url[got] != 0).all(), regime
    idx = mse.ScalarQuantizerIndex(D)
    x32 = orc.f16_to_f32(ix.rows)
    for lo in range(0, ix.N, 1024):
        idx.add(x32[lo:lo + 1024])
    a, b = idx.search(ix.qs, ix.K, allow=dev), idx.search(ix.qs, ix.K, allow=host)
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.distances, b.distances) and mask[a.labels].all()
    check(dev, mask, "unchanged by its consumers")


# ---- 5. delete by predicate -----------------------------------------------------------------------------------------------------

def test_delete_by_predicate(gpu, mse, orc):
    """delete_rows under from_descriptors(codes, {3: (0, t)}) on one upload, under the numpy mask on its twin: the same graph, the same
    deleted map, the same stats."""
    ix = Index3k(mse, orc)
    t = 70
    mask = ix.desc[:, 3] <= t
    assert ix.N // 5 < mask.sum() < ix.N // 3
    g1, g2 = ix.graph(), ix.graph()
    f = mse.RowFilter.from_descriptors(ix.gcodes, {3: (0, t)})
    check(f, mask, "the delete set")
    st1 = g1.delete_rows(ix.searcher, f, ix.mcfg)
    st2 = g2.delete_rows(ix.searcher, mask, ix.mcfg)
    assert st1 == st2 and st1["deleted"] == int(mask.sum()) and st1["lists_rewritten"] > 0
    h1, h2 = g1.to_host(), g2.to_host()
    used = np.arange(h1.adj.shape[1])[None, :] < h1.deg[:, None]
    assert np.array_equal(h1.deg, h2.deg) and np.array_equal(h1.adj[used], h2.adj[used])
    assert np.array_equal(g1.deleted(), mask) and np.array_equal(g2.deleted(), mask)
    check(g1.live_filter(), ~mask, "live after the delete")
    check(~f, ~mask, "the complement of the delete set")
    g1.close()
    g2.close()


# ---- 6. bits that already are on the device -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 8193])
def test_from_device_bits(gpu, mse, n):
    import torch
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.5
    mask[n - 1] = True
    bits = np.packbits(mask, bitorder="little")
    assert n % 8 == 1
    bits[-1] |= 0xFE                                                         # garbage past n_rows in the last byte
    t = torch.from_numpy(bits).cuda()
    torch.cuda.synchronize()
    f = mse.RowFilter.from_device_bits(t.data_ptr(), n)
    check(f, mask, "from device bits")
    host = mse.RowFilter(mask)
    assert np.array_equal(f.to_mask(), host.to_mask()) and np.array_equal(f.ids(), host.ids()) and f.count == host.count
    assert np.array_equal(t.cpu().numpy(), bits)                             # the source is only read
    check(~f, ~mask, "its complement")


# ---- 7. errors make nothing and name the check --------------------------------------------------------------------------------------

def test_errors_make_nothing(gpu, mse, orc):
    from mse import ffi
    L = ffi.lib()
    n = 300
    rng = np.random.default_rng(9)
    m = rng.random(n) < 0.5
    a, longer = mse.RowFilter(m), mse.RowFilter(np.ones(n + 1, bool))
    base = orc.gen_rows_f16(SEED_BASE, 0, n)
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    q = orc.gen_rows_f16(SEED_QUERY, 0, 1)[0]
    qp = q.ctypes.data_as(ffi.u16p)
    bare = mse.Codes(np.zeros((n, 8), np.uint8), None)
    lo, hi = np.zeros(8, np.uint8), np.full(8, 255, np.uint8)
    lop, hip = lo.ctypes.data_as(ffi.u8p), hi.ctypes.data_as(ffi.u8p)
    creators = [
        (lambda: L.mse_filter_combine(None, a._h, 0), "null filter"),
        (lambda: L.mse_filter_combine(a._h, None, 1), "null filter"),
        (lambda: L.mse_filter_combine(a._h, a._h, 4), "unknown op"),
        (lambda: L.mse_filter_combine(a._h, a._h, -1), "unknown op"),
        (lambda: L.mse_filter_not(None, 0), "null filter"),
        (lambda: L.mse_filter_not(a._h, n - 1), "is below the filter's"),
        (lambda: L.mse_filter_from_descriptors(bare._h, lop, hip), "no descriptor bytes"),
        (lambda: L.mse_filter_from_descriptors(None, lop, hip), "null codes"),
        (lambda: L.mse_filter_from_scores(s._h, qp, 0, longer._h), "longer than the base"),
        (lambda: L.mse_filter_from_scores(s._h, None, 0, None), "null query"),
        (lambda: L.mse_filter_from_scores(None, qp, 0, None), "null searcher"),
        (lambda: L.mse_filter_from_bits_dev(None, 5), "null bitmap"),
    ]
    for call, text in creators:
        assert call() is None, text
        assert text in ffi.last_error(), (text, ffi.last_error())
    with pytest.raises(mse.MseError):
        a.invert(n - 1)
    with pytest.raises(TypeError):
        a & m
    with pytest.raises(TypeError):
        mse.RowFilter.from_scores(s, q, 0, within=m)
    out = np.full(n + 8, 0x5A5A5A5A, np.uint32)
    op = out.ctypes.data_as(ffi.u32p)
    for first, cnt in ((0, a.count + 1), (a.count, 1), (a.count + 1, 0), (2 ** 63, 2 ** 63)):
        assert L.mse_filter_read_ids(a._h, first, cnt, op) != 0
        assert "past the filter's" in ffi.last_error() and (out == 0x5A5A5A5A).all()
    assert L.mse_filter_read_ids(None, 0, 0, op) != 0 and "null filter" in ffi.last_error()
    assert L.mse_filter_read_ids(a._h, a.count, 0, op) == 0 and (out == 0x5A5A5A5A).all()
    assert L.mse_filter_to_bits(a._h, None) != 0 and "null buffer" in ffi.last_error()
    assert L.mse_filter_to_bits(None, out.ctypes.data_as(ffi.u8p)) != 0 and "null filter" in ffi.last_error()
    # to_bits writes exactly (n_rows + 7) / 8 bytes; read_ids exactly n ids
    buf = np.full(n // 8 + 9, 0xA5, np.uint8)
    assert L.mse_filter_to_bits(a._h, buf.ctypes.data_as(ffi.u8p)) == 0
    assert (buf[(n + 7) // 8:] == 0xA5).all() and np.array_equal(buf[:(n + 7) // 8], np.packbits(m, bitorder="little"))
    assert L.mse_filter_read_ids(a._h, 3, 5, op) == 0
    assert np.array_equal(out[:5], np.flatnonzero(m)[3:8]) and (out[5:] == 0x5A5A5A5A).all()
    assert np.array_equal(a.ids(3, 5), np.flatnonzero(m)[3:8])
    check(a, m, "the operand of the failed calls")
