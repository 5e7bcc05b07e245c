"""Row filters on the shard group (include/mse.h mse_filter_slice / _concat / mse_shard_filter and the *_filtered searches of
mse_shard_group / mse_comm).  Everything is compared by equality: slice and concat against numpy on boolean masks; the sharded
filtered searches against the unsharded filtered calls (themselves pinned against the oracle) and against the CPU oracle directly."""
import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY, make_pq

pytestmark = pytest.mark.gpu
D, N, K = 1152, 2999, 10
NONE, LOWEST = 0xFFFFFFFF, np.iinfo(np.int64).min
SCALES = np.array([0.5, 0, -0.25, 1.0], np.float32) / np.float32(512)


# ---- slice and concat against numpy -----------------------------------------------------------------------------------------------
N_SRC = 17_000


def source_masks():
    rng = np.random.default_rng(61)
    ends = np.zeros(N_SRC, bool)
    ends[[0, N_SRC - 1]] = True
    return {"ones": np.ones(N_SRC, bool), "zeros": np.zeros(N_SRC, bool), "ends": ends, "half": rng.random(N_SRC) < 0.5,
            "sparse": rng.random(N_SRC) < 1e-3}


@pytest.fixture(scope="module")
def sources(gpu, mse):
    masks = source_masks()
    return masks, {name: mse.RowFilter(m) for name, m in masks.items()}


def np_slice(m, first, n_rows):
    out = np.zeros(n_rows, bool)
    part = m[first:first + n_rows]
    out[:len(part)] = part
    return out


def check_filter(f, want):
    """to_mask, count, ids, and the tail word through the complement (a stray bit past the length would show in its count)"""
    n = len(want)
    assert len(f) == n
    assert np.array_equal(f.to_mask(), want)
    assert f.count == int(want.sum())
    assert np.array_equal(f.ids(), np.flatnonzero(want).astype(np.uint32))
    inv = ~f
    assert inv.count == n - f.count
    inv.close()


@pytest.mark.parametrize("shift", [0, 1, 31])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 255, 256, 257, 8191, 8192, 8193, 16385])
def test_slice_equals_numpy(sources, mse, shift, n_rows):
    """first_row % 32 in {0, 1, 31}; lengths around the word, the 256-row tile and the 8192-row compaction block"""
    masks, filters = sources
    def last_at_most(limit):                                           # the largest first row <= limit with first_row % 32 == shift
        return limit - (limit - shift) % 32
    half_in = last_at_most(N_SRC - (n_rows + 1) // 2)                  # half inside the source, half past its length
    on_last = last_at_most(N_SRC - 1)                                  # the source's last rows, then past its length
    firsts = [shift, 64 + shift, half_in, on_last, N_SRC // 32 * 32 + 32 + shift]     # ... and wholly past it
    assert all(f % 32 == shift for f in firsts) and on_last + 32 >= N_SRC > on_last and firsts[-1] >= N_SRC
    assert n_rows < 64 or half_in + n_rows > N_SRC
    for name, f in filters.items():
        for first in firsts:
            s = f.slice(first, n_rows)
            check_filter(s, np_slice(masks[name], first, n_rows))
            if first >= N_SRC:
                assert s.count == 0 and not s.to_mask().any()
            s.close()


def test_slice_on_the_named_device_and_errors(sources, mse):
    masks, filters = sources
    s = filters["half"].slice(750, 750, device=0)                       # the same device named explicitly
    check_filter(s, masks["half"][750:1500])
    s.close()
    with pytest.raises(mse.MseError, match="n_rows"):
        filters["half"].slice(0, 0)
    with pytest.raises(mse.MseError, match="device"):
        filters["half"].slice(0, 10, device=99)
    from mse import ffi
    assert not ffi.lib().mse_filter_slice(None, 0, 10, -1) and "null" in ffi.last_error()


def test_concat_equals_numpy(sources, mse):
    masks, filters = sources
    m = masks["half"]
    # parts that share a boundary word, a gap between parts, parts given out of order
    a, b, c = filters["half"].slice(5, 45), filters["ones"].slice(0, 30), filters["half"].slice(1000, 8300)
    want = np.zeros(9000, bool)
    want[3:48], want[48:78], want[130:8430] = m[5:50], True, m[1000:9300]
    got = mse.RowFilter.concat([c, a, b], [130, 3, 48], 9000)
    check_filter(got, want)
    got.close()
    # round trip at the group's split (2 999 rows over 4 shards: 750, 1 500, 2 250) and at odd cuts of a longer filter
    for n, cuts in ((N, [0, 750, 1500, 2250, N]), (N_SRC, [0, 1, 33, 8192, 8193 + 31, 16385, N_SRC])):
        for name in ("half", "ends", "sparse", "ones"):
            whole = filters[name].slice(0, n)
            parts = [whole.slice(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
            back = mse.RowFilter.concat(parts, cuts[:-1], n)
            check_filter(back, masks[name][:n])
            for p in parts + [back, whole]:
                p.close()
    # errors: overlapping parts, a part past n_rows, n_rows = 0, null arguments -- and nothing is made
    with pytest.raises(mse.MseError, match="overlap"):
        mse.RowFilter.concat([a, b], [3, 47], 9000)
    with pytest.raises(mse.MseError, match="past"):
        mse.RowFilter.concat([a, b], [3, 8971], 9000)
    with pytest.raises(mse.MseError, match="n_rows"):
        mse.RowFilter.concat([], [], 0)
    from mse import ffi
    import ctypes as C
    assert not ffi.lib().mse_filter_concat(None, None, 2, 100, -1) and "null" in ffi.last_error()
    hs, fr = (C.c_void_p * 2)(a._h, None), (C.c_uint64 * 2)(0, 64)
    assert not ffi.lib().mse_filter_concat(hs, fr, 2, 100, -1) and "null" in ffi.last_error()
    for p in (a, b, c):
        p.close()


# ---- brute force ------------------------------------------------------------------------------------------------------------------
def group_masks(n, G, mse):
    """the filters of the issue over n rows split into G shards"""
    rng = np.random.default_rng(62 + G)
    bounds = [mse.shard_range(n, g, G) for g in range(G)]
    half = rng.random(n) < 0.5
    no_shard = half.copy()
    lo, hi = bounds[G // 2]
    no_shard[lo:hi] = False                                               # one shard entirely disallowed (G = 1: nothing allowed)
    few = np.zeros(n, bool)
    few[rng.choice(n, K - 3, replace=False)] = True                       # fewer than k allowed overall
    ends = np.zeros(n, bool)
    for lo, hi in bounds:
        ends[[lo, lo + 1, hi - 2, hi - 1]] = True                         # allowed rows only at both ends of each shard
    short = rng.random(n - 801) < 0.5                                     # shorter than the group: the rows past it are excluded
    return {"half": half, "no_shard": no_shard, "few": few, "ends": ends, "short": short}


def full(mask, n):
    m = np.zeros(n, bool)
    m[:len(mask)] = mask
    return m


def oracle_filtered(orc, base, q, k, mask):
    """the oracle on rows[allowed], ids mapped back, padded"""
    ids = np.flatnonzero(full(mask, len(base)))
    nq = len(q)
    ws, wi = np.full((nq, k), LOWEST, np.int64), np.full((nq, k), NONE, np.uint32)
    kk = min(k, len(ids))
    if kk:
        s, i = orc.bruteforce_topk(base[ids], q, kk)
        ws[:, :kk], wi[:, :kk] = s, ids[i].astype(np.uint32)
    return ws, wi


@pytest.fixture(scope="module")
def flat(gpu, mse, orc):
    base = orc.gen_rows_f16(SEED_BASE, 0, N)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 9)
    vecs = mse.VectorList.from_f16s(base, D)
    return base, q, mse.Searcher(vecs)


@pytest.mark.parametrize("nq", [1, 9])
@pytest.mark.parametrize("G", [1, 3, 4])
def test_sharded_filtered_bruteforce_equals_the_unsharded_call_and_the_oracle(flat, mse, orc, G, nq):
    base, q, whole = flat
    q = q[:nq]
    grp = mse.ShardGroup(G, D, devices=[0] * G)
    grp.load_host(base)
    for name, mask in group_masks(N, G, mse).items():
        rf = mse.RowFilter(mask)
        sf = grp.filter(rf)
        assert sf.n_shards == G and sf.count == int(mask.sum())
        for g in range(G):
            lo, hi = mse.shard_range(N, g, G)
            assert np.array_equal(sf.shard(g).to_mask(), full(mask, N)[lo:hi]), (name, g)
        glob = sf.to_global()
        assert np.array_equal(glob.to_mask(), full(mask, N))
        glob.close()
        ws, wi = oracle_filtered(orc, base, q, K, mask)
        if name in ("few", "no_shard") and mask.sum() < K:
            assert (wi[:, int(mask.sum()):] == NONE).all() and (ws[:, int(mask.sum()):] == LOWEST).all()
        for mode in (mse.MODE_EXACT, mse.MODE_MFMA, mse.MODE_AUTO):
            us, ui = whole.bruteforce_topk(q, K, mode, allow=rf)
            gs, gi = grp.bruteforce_topk_filtered(sf, q, K, mode)
            assert np.array_equal(gi, ui) and np.array_equal(gs, us), (name, mode)
            assert np.array_equal(gi, wi) and np.array_equal(gs, ws), (name, mode)
        sf.close()
        rf.close()
    grp.close()


def test_sharded_filtered_bruteforce_device_form(flat, mse, orc):
    import torch
    base, q, _ = flat
    mask = group_masks(N, 4, mse)["half"]
    grp = mse.ShardGroup(4, D, devices=[0] * 4)
    grp.load_host(base)
    sf = grp.filter(mse.RowFilter(mask))
    qd = torch.from_numpy(q.view(np.int16)).cuda()
    out_s = torch.empty((len(q), K), dtype=torch.int64, device="cuda")
    out_i = torch.empty((len(q), K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    grp.bruteforce_topk_filtered_dev(sf, qd.data_ptr(), len(q), K, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)
    ws, wi = oracle_filtered(orc, base, q, K, mask)
    assert np.array_equal(out_s.cpu().numpy(), ws) and np.array_equal(out_i.cpu().numpy().view(np.uint32), wi)
    sf.close()
    grp.close()


def test_filtered_ties_across_shards_break_by_lower_global_id(gpu, mse, orc):
    # the same row everywhere: equal scores in different shards come back in ascending global id, among the allowed rows only
    row = orc.gen_rows_f16(SEED_BASE, 7, 1)
    base = np.repeat(row, 64, axis=0)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 2)
    mask = np.zeros(64, bool)
    mask[[3, 14, 15, 16, 17, 31, 32, 33, 47, 48, 50, 63]] = True            # both sides of the boundaries at 16, 32 and 48
    grp = mse.ShardGroup(4, D, devices=[0] * 4)
    grp.load_host(base)
    sf = grp.filter(mse.RowFilter(mask))
    for mode in (mse.MODE_MFMA, mse.MODE_EXACT, mse.MODE_AUTO):
        s, i = grp.bruteforce_topk_filtered(sf, q, 10, mode)
        assert i.tolist() == [np.flatnonzero(mask)[:10].tolist()] * 2, mode
        ws, wi = oracle_filtered(orc, base, q, 10, mask)
        assert np.array_equal(s, ws) and np.array_equal(i, wi)
    sf.close()
    grp.close()


def test_filter_over_shards_set_at_odd_first_rows(flat, mse, orc):
    """set_shard_device at first rows 31 and 33 + n0: neither is a multiple of 32, and two global rows between the shards belong to nobody"""
    import torch
    base, q, _ = flat
    n0, n1 = 1000, 777
    f0, f1 = 31, 33 + n0
    end = f1 + n1
    t0 = torch.from_numpy(base[:n0].view(np.int16).copy()).cuda()
    t1 = torch.from_numpy(base[n0:n0 + n1].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    grp = mse.ShardGroup(2, D, devices=[0, 0])
    grp.set_shard_device(0, t0.data_ptr(), n0, f0)
    grp.set_shard_device(1, t1.data_ptr(), n1, f1)
    mask = np.random.default_rng(63).random(end) < 0.5
    mask[[f0, f0 + n0 - 1, f0 + n0, f0 + n0 + 1, f1, end - 1]] = True        # the shards' end rows and the two rows in the gap
    rf = mse.RowFilter(mask)
    sf = grp.filter(rf)
    assert np.array_equal(sf.shard(0).to_mask(), mask[f0:f0 + n0]) and np.array_equal(sf.shard(1).to_mask(), mask[f1:end])
    held = np.zeros(end, bool)
    held[f0:f0 + n0] = held[f1:end] = True
    glob = sf.to_global()
    assert np.array_equal(glob.to_mask(), mask & held)                       # rows nobody holds read as zero
    glob.close()
    rows = np.zeros((end, D), np.uint16)                                     # the index as one array of global rows
    rows[f0:f0 + n0], rows[f1:end] = base[:n0], base[n0:n0 + n1]
    ws, wi = oracle_filtered(orc, rows, q, K, mask & held)
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA):
        gs, gi = grp.bruteforce_topk_filtered(sf, q, K, mode)
        assert np.array_equal(gi, wi) and np.array_equal(gs, ws), mode
    longer = mse.RowFilter(np.ones(end + 1, bool))
    with pytest.raises(mse.MseError, match="longer"):
        grp.filter(longer)
    sf.close()
    grp.close()


# ---- PQ scan and graph: one small index per group size ----------------------------------------------------------------------------
class Ann:
    """N clustered rows over G logical shards: a codec, per-shard codes (+ descriptors) made from the shard's resident rows, a small
    graph per shard with has_url flags and an entry table; the unsharded vectors and codes beside them."""

    def __init__(self, mse, orc, G, seed, has_url=True):
        from test_gpu_pq_index_graph import clustered_rows, knn_graph
        rng = np.random.default_rng(seed)
        self.G = G
        self.x = clustered_rows(orc, N, n_centres=40, seed=seed)
        self.base = orc.f16_bits(self.x)
        cents, T, dpc, _ = make_pq(orc, seed=seed)
        self.pq = mse.ProductQuantizer(cents, T, dpc, D)
        self.desc = rng.integers(0, 256, size=(N, 4), dtype=np.uint8)
        self.vecs = mse.VectorList.from_f16s(self.base, D)
        self.whole = mse.Searcher(self.vecs)
        self.whole_codes = mse.Codes.quantize_base(self.pq, self.vecs, self.desc)
        self.grp = mse.ShardGroup(G, D, devices=[0] * G)
        self.grp.load_host(self.base)
        self.bounds = [mse.shard_range(N, g, G) for g in range(G)]
        self.codes, self.graphs, self.host = [], [], []
        for g, (lo, hi) in enumerate(self.bounds):
            codes = mse.Codes.quantize_base(self.pq, self.grp.base(g), self.desc[lo:hi])
            self.grp.attach_pq(g, self.pq, codes)
            self.codes.append(codes)
            adj, degs = knn_graph(self.x[lo:hi], 12, rng)
            url = (rng.random(hi - lo) > 0.1).astype(np.uint8) if has_url else None
            entries = np.sort(rng.choice(hi - lo, 16, replace=False)).astype(np.uint32)
            self.host.append((adj, degs, url, entries))
            self.attach_fresh_graph(mse, g)
        self.qs = clustered_rows(orc, 9, n_centres=40, seed=seed + 500).astype(np.float32)
        self.qh = orc.f16_bits(self.qs)

    def attach_fresh_graph(self, mse, g):
        adj, degs, url, entries = self.host[g]
        dg = mse.DeviceGraph(mse.IndexGraph(adj, degs), url)
        mse.set_entries(dg, self.grp.base(g), entries)
        self.grp.attach_graph(g, dg)
        if g < len(self.graphs):
            self.graphs[g] = dg
        else:
            self.graphs.append(dg)
        return dg


@pytest.fixture(scope="module")
def anns(gpu, mse, orc):
    made = {}

    def get(G):
        if G not in made:
            made[G] = Ann(mse, orc, G, 70 + G)
        return made[G]
    return get


@pytest.mark.parametrize("G", [1, 3, 4])
def test_sharded_filtered_pq_scan_equals_the_unsharded_call_bit_for_bit(anns, mse, G):
    a = anns(G)
    masks = group_masks(N, G, mse)
    rng = np.random.default_rng(64)
    under_r = np.zeros(N, bool)
    under_r[rng.choice(N, 30, replace=False)] = True                         # k <= allowed < r = 64
    cases = {"half": masks["half"], "no_shard": masks["no_shard"], "few": masks["few"], "under_r": under_r, "short": masks["short"]}
    for name, mask in cases.items():
        rf = mse.RowFilter(mask)
        sf = a.grp.filter(rf)
        for r in (K, 64):
            for sc in (None, SCALES):
                for nq in (9, 1):
                    want_s, want_i = a.pq.scan_topk_batch_filtered(a.whole_codes, rf, a.qs[:nq], r, K, a.whole, sc, "scan")
                    if name == "few":
                        assert (want_i[:, K - 3:] == NONE).all() and (want_i[:, :K - 3] != NONE).all()
                    for mode in ("scan", "list", "auto"):
                        got_s, got_i = a.grp.pq_scan_topk_filtered(sf, a.qs[:nq], r, K, sc, mode)
                        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, r, sc is not None, nq, mode)
                    assert full(mask, N)[want_i[want_i != NONE]].all()
        sf.close()
        rf.close()


def sorted_cut(ids, sc, k):
    order = sorted(range(len(ids)), key=lambda j: (-int(sc[j]), int(ids[j])))[:k]
    wi, ws = np.full(k, NONE, np.uint32), np.full(k, LOWEST, np.int64)
    wi[:len(order)] = np.asarray(ids, np.uint32)[order]
    ws[:len(order)] = np.asarray(sc, np.int64)[order]
    return wi, ws


def oracle_shard_answer(a, orc, mse, g, local_mask, regime, scales, beam, L, k):
    """one shard's filtered answer by the CPU oracle: GRAPH = the reference's search over an index whose has_url is (has_url AND allowed);
    LIST = every eligible row scored, biased and sorted; AUTO = whichever the shard's own plan names, at its search_list"""
    lo, hi = a.bounds[g]
    adj, degs, url, entries = a.host[g]
    rows, desc = a.base[lo:hi], a.desc[lo:hi]
    eligible = local_mask & (url.astype(bool) if url is not None else True)
    if regime == "auto":
        regime, L = mse.filtered_plan(hi - lo, int(local_mask.sum()), L)
    nq = len(a.qh)
    out_i, out_s = np.full((nq, k), NONE, np.uint32), np.full((nq, k), LOWEST, np.int64)
    if regime == "graph":
        _, best = orc.bruteforce_topk(rows[entries], a.qh, 1)
    for q in range(nq):
        if regime == "list":
            ids = np.flatnonzero(eligible)
            sc = orc.score_all(rows, a.qh[q])[ids]
            if scales is not None:
                sc = sc + np.array([orc.descriptor_product(scales, desc, int(i)) for i in ids], np.int64)
        else:
            _, ids, sc, _, _ = orc.disk_greedy_search(rows, adj, degs, np.zeros((hi - lo, 64), np.uint8), desc, int(entries[best[q, 0]]), a.qh[q],
                                                      np.zeros(64 * 256, np.float32), scales, True, beam, L, eligible.astype(np.uint8))
        out_i[q], out_s[q] = sorted_cut(ids, sc, k)
    return out_i, out_s


@pytest.mark.parametrize("G", [1, 4])
def test_sharded_filtered_graph_query_equals_the_merge_of_the_per_shard_answers(anns, mse, orc, G):
    a = anns(G)
    beam, L = 2, 24
    masks = group_masks(N, G, mse)
    tenth = np.random.default_rng(65).random(N) < 0.012                     # about 9 rows per shard of 750: AUTO plans LIST there
    for name, mask in (("half", masks["half"]), ("few", masks["few"]), ("tenth", tenth), ("no_shard", masks["no_shard"])):
        rf = mse.RowFilter(mask)
        sf = a.grp.filter(rf)
        for regime in ("graph", "list", "auto"):
            for sc in (None, SCALES):
                sc_q = None if sc is None else np.ascontiguousarray(np.broadcast_to(sc, (len(a.qh), 4)))
                got_s, got_i = a.grp.query_topk_filtered(sf, a.qh, K, None, sc_q, True, beam, L, regime)
                dev_s = np.full((len(a.qh), G * K), LOWEST, np.int64)
                dev_i = np.full((len(a.qh), G * K), NONE, np.uint32)
                orc_s, orc_i = dev_s.copy(), dev_i.copy()
                for g, (lo, hi) in enumerate(a.bounds):
                    part = sf.shard(g)
                    # the direct per-shard call
                    wi, ws, _ = mse.disk_query_topk(a.grp.searcher(g), a.pq, a.codes[g], a.graphs[g], a.qh, K, None, None, sc_q, True, beam, L,
                                                    filter=part, regime=regime)
                    dev_s[:, g * K:(g + 1) * K] = ws
                    dev_i[:, g * K:(g + 1) * K] = np.where(wi == NONE, wi, wi + np.uint32(lo))
                    oi, os_ = oracle_shard_answer(a, orc, mse, g, full(mask, N)[lo:hi], regime, sc, beam, L, K)
                    orc_s[:, g * K:(g + 1) * K] = os_
                    orc_i[:, g * K:(g + 1) * K] = np.where(oi == NONE, oi, oi + np.uint32(lo))
                want_s, want_i = mse.shard.merge_topk_numpy(dev_s, dev_i, K)
                assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, regime, sc is not None)
                want_s, want_i = mse.shard.merge_topk_numpy(orc_s, orc_i, K)
                assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, regime, sc is not None, "oracle")
        sf.close()
        rf.close()


def test_list_regime_without_has_url_is_the_sharded_filtered_bruteforce_plus_the_bias(gpu, mse, orc):
    a = Ann(mse, orc, 3, 81, has_url=False)
    masks = group_masks(N, 3, mse)
    for name in ("half", "few", "ends"):
        sf = a.grp.filter(mse.RowFilter(masks[name]))
        bs, bi = a.grp.bruteforce_topk_filtered(sf, a.qh, K, mse.MODE_EXACT)
        ls, li = a.grp.query_topk_filtered(sf, a.qh, K, None, None, True, 2, 24, "list")
        assert np.array_equal(li, bi) and np.array_equal(ls, bs), name
        if name == "few":           # every allowed row is in the answer, so the biased answer is the unbiased one + the bias, re-sorted
            sc_q = np.ascontiguousarray(np.broadcast_to(SCALES, (len(a.qh), 4)))
            ls2, li2 = a.grp.query_topk_filtered(sf, a.qh, K, None, sc_q, True, 2, 24, "list")
            for q in range(len(a.qh)):
                ids = bi[q][bi[q] != NONE]
                biased = bs[q][:len(ids)] + np.array([orc.descriptor_product(SCALES, a.desc, int(i)) for i in ids], np.int64)
                wi, ws = sorted_cut(ids, biased, K)
                assert np.array_equal(li2[q], wi) and np.array_equal(ls2[q], ws)
        sf.close()
    a.grp.close()


def test_live_filter_keeps_deleted_rows_out_of_every_filtered_group_call(gpu, mse, orc):
    G = 4
    a = Ann(mse, orc, G, 82, has_url=False)
    qs, qh = a.qs, a.qh
    before_bf = a.grp.bruteforce_topk(qh, K, mse.MODE_EXACT)
    before_pq = a.grp.pq_scan_topk(qs, 64, K)
    # delete, through the graphs of shards 1 and 3, the best rows of the unfiltered answers that live there (entry nodes stay)
    dead = np.zeros(N, bool)
    for g in (1, 3):
        lo, hi = a.bounds[g]
        cand = np.unique(np.concatenate([before_bf[1].ravel(), before_pq[1].ravel()]))
        cand = cand[(cand >= lo) & (cand < hi)]
        local = np.setdiff1d(cand - lo, a.host[g][3])[:20].astype(np.uint32)
        extra = np.setdiff1d(np.arange(hi - lo - 40, hi - lo, dtype=np.uint32), a.host[g][3])   # the shard's last rows too
        local = np.union1d(local, extra).astype(np.uint32)
        assert len(local) > 20
        st = a.graphs[g].delete_rows(a.grp.searcher(g), local, mse.IndexBuildConfig(r=12, l=24, maxc=100))
        assert st["deleted"] == len(local)
        dead[lo + local] = True
    live = a.grp.live_filter()
    glob = live.to_global()
    assert np.array_equal(glob.to_mask(), ~dead) and live.count == N - int(dead.sum())
    glob.close()
    for g in range(G):
        lo, hi = a.bounds[g]
        assert np.array_equal(live.shard(g).to_mask(), ~dead[lo:hi])
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA, mse.MODE_AUTO):
        s, i = a.grp.bruteforce_topk_filtered(live, qh, K, mode)
        assert not dead[i].any()
        ws, wi = oracle_filtered(orc, a.base, qh, K, ~dead)
        assert np.array_equal(i, wi) and np.array_equal(s, ws)
    for mode in ("scan", "list", "auto"):
        s, i = a.grp.pq_scan_topk_filtered(live, qs, 64, K, None, mode)
        assert (i != NONE).all() and not dead[i].any()
    for regime in ("graph", "list", "auto"):
        s, i = a.grp.query_topk_filtered(live, qh, K, None, None, True, 2, 24, regime)
        assert (i != NONE).all() and not dead[i].any()
    # nothing existing changed: the unfiltered flat calls answer as before the deletes, dead rows included
    after_bf = a.grp.bruteforce_topk(qh, K, mse.MODE_EXACT)
    after_pq = a.grp.pq_scan_topk(qs, 64, K)
    assert np.array_equal(after_bf[0], before_bf[0]) and np.array_equal(after_bf[1], before_bf[1]) and dead[after_bf[1]].any()
    assert np.array_equal(after_pq[0], before_pq[0]) and np.array_equal(after_pq[1], before_pq[1]) and dead[after_pq[1]].any()
    # a shard without a graph
    a.grp.attach_graph(2, None)
    with pytest.raises(mse.MseError, match="graph"):
        a.grp.live_filter()
    live.close()
    a.grp.close()


# ---- stale and foreign filters ----------------------------------------------------------------------------------------------------
def test_stale_and_foreign_shard_filters_are_refused_without_writing(anns, flat, mse):
    a = anns(4)
    base = flat[0]
    mask = group_masks(N, 4, mse)["half"]
    rf = mse.RowFilter(mask)
    other = mse.ShardGroup(4, D, devices=[0] * 4)
    other.load_host(base)
    foreign = other.filter(rf)
    stale = a.grp.filter(rf)                # made for the group's rows as they are now; the rows are re-loaded below
    good_before = a.grp.bruteforce_topk_filtered(stale, a.qh, K)

    def refused(grp, sf, match):
        s0 = np.full((len(a.qh), K), 12345, np.int64)
        i0 = np.full((len(a.qh), K), 54321, np.uint32)
        import ctypes as C
        from mse import ffi
        from mse.vector import _p
        L = ffi.lib()
        q32 = a.qs
        calls = [
            lambda: L.mse_shard_group_search_filtered(grp._h, sf, _p(a.qh, C.c_uint16), len(a.qh), K, 0, _p(s0, C.c_int64), _p(i0, C.c_uint32)),
            lambda: L.mse_shard_group_pq_scan_topk_filtered(grp._h, sf, _p(q32, C.c_float), None, len(q32), 64, K, 0, _p(s0, C.c_int64), _p(i0, C.c_uint32)),
            lambda: L.mse_shard_group_query_topk_filtered(grp._h, sf, _p(a.qh, C.c_uint16), None, None, len(a.qh), 1, 2, 24, K, 0, _p(s0, C.c_int64),
                                                          _p(i0, C.c_uint32)),
        ]
        for call in calls:
            assert call() != 0
            assert match in ffi.last_error(), ffi.last_error()
            assert (s0 == 12345).all() and (i0 == 54321).all()

    refused(a.grp, foreign._h, "another group")                  # a shard filter from another group
    refused(a.grp, None, "null shard filter")
    with pytest.raises(TypeError):
        a.grp.bruteforce_topk_filtered(rf, a.qh, K)               # a RowFilter is not a ShardFilter
    # wrong shard length: per-shard filters that do not fit are refused when the shard filter is made
    parts = [stale.shard(g) for g in range(4)]
    wrong = parts[:3] + [parts[0]]                                # shard 3 holds 749 rows, shard 0's filter has 750
    with pytest.raises(mse.MseError, match="rows"):
        a.grp.filter_from_local(wrong)
    with pytest.raises(ValueError):
        a.grp.filter_from_local(parts[:3])
    again = a.grp.filter_from_local(parts)                        # ... and the fitting ones give the same answers
    got = a.grp.bruteforce_topk_filtered(again, a.qh, K)
    assert np.array_equal(got[0], good_before[0]) and np.array_equal(got[1], good_before[1]) and again.count == stale.count
    # the same rows loaded again: a new layout, so every filter from before it is stale
    a.grp.load_host(a.base)
    refused(a.grp, stale._h, "before the group's rows were replaced")
    refused(a.grp, again._h, "before the group's rows were replaced")
    fresh = a.grp.filter(rf)
    got = a.grp.bruteforce_topk_filtered(fresh, a.qh, K)
    assert np.array_equal(got[0], good_before[0]) and np.array_equal(got[1], good_before[1])
    for g in range(4):                                            # (the re-load dropped nothing: codes and graphs stay attached)
        assert len(a.grp.base(g)) == a.bounds[g][1] - a.bounds[g][0]
    for x in (foreign, stale, again, fresh, rf):
        x.close()
    other.close()


# ---- the process-per-GPU forms as a world of one -----------------------------------------------------------------------------------
def test_comm_world_of_one_filtered_paths_equal_the_single_shard_group(anns, mse, orc):
    import torch
    a = anns(1)
    nq, r, first = len(a.qh), 64, 1000
    mask = group_masks(N, 1, mse)["half"]
    glob = mse.RowFilter(full(np.concatenate([np.zeros(first, bool), mask]), first + N))
    local = glob.slice(first, N)                                   # the rank's LOCAL filter, cut from the global one at its first row
    assert np.array_equal(local.to_mask(), mask)
    sf = a.grp.filter(local)
    comm = mse.Comm(mse.Comm.unique_id(), 0, 1)
    out_s = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    out_i = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    qd = torch.from_numpy(a.qh.view(np.int16)).cuda()
    torch.cuda.synchronize()

    def got():
        torch.cuda.synchronize()
        return out_s.cpu().numpy(), out_i.cpu().numpy().view(np.uint32)

    def lifted(i):
        return np.where(i == NONE, i, i + np.uint32(first))
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA, mse.MODE_AUTO):
        comm.search_filtered_dev(a.whole, local, qd.data_ptr(), nq, K, out_s.data_ptr(), out_i.data_ptr(), mode, id_offset=first)
        ws, wi = a.grp.bruteforce_topk_filtered(sf, a.qh, K, mode)
        s, i = got()
        assert np.array_equal(s, ws) and np.array_equal(i, lifted(wi)), mode
    for mode in ("scan", "list", "auto"):
        comm.pq_scan_topk_filtered(a.pq, a.whole_codes, a.whole, local, a.qs, r, K, first, out_s.data_ptr(), out_i.data_ptr(), SCALES, mode)
        ws, wi = a.grp.pq_scan_topk_filtered(sf, a.qs, r, K, SCALES, mode)
        s, i = got()
        assert np.array_equal(s, ws) and np.array_equal(i, lifted(wi)), mode
    for regime in ("graph", "list", "auto"):
        comm.query_topk_filtered(a.whole, a.graphs[0], local, a.qh, K, first, out_s.data_ptr(), out_i.data_ptr(), disable_pq=True, beamwidth=2,
                                 search_list=24, regime=regime)
        ws, wi = a.grp.query_topk_filtered(sf, a.qh, K, None, None, True, 2, 24, regime)
        s, i = got()
        assert np.array_equal(s, ws) and np.array_equal(i, lifted(wi)), regime
    from mse import ffi
    assert ffi.lib().mse_comm_search_filtered_dev(comm._h, a.whole._h, None, qd.data_ptr(), nq, K, 0, 0, out_s.data_ptr(), out_i.data_ptr()) != 0
    assert "null filter" in ffi.last_error()
    comm.close()
    sf.close()
