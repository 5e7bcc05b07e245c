"""Grouped ("collapse") search on the shard group (include/mse.h "grouped search across the shards"): mse_groups_slice / mse_groups_read,
the grouped merge (mse_merge_topk_packed_grouped_dev) and the three *_grouped searches of mse_shard_group.  Everything is compared by
equality: the slice against the numpy restatement of its canonical rule, the merge against a numpy collapse of hand-made blocks, the
sharded brute force against the unsharded grouped call and the collapse of the oracle's full ranking, the graph and PQ paths against
the numpy collapse -- by the GLOBAL grouping -- of everything the ungrouped sharded calls return."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY
from test_gpu_shard_filter import Ann, SCALES, group_masks

pytestmark = pytest.mark.gpu
D, N, K = 1152, 2999, 10
NONE, LOWEST = 0xFFFFFFFF, np.iinfo(np.int64).min
CUTS4 = [0, 750, 1500, 2250]


# ---- the groupings ------------------------------------------------------------------------------------------------------------------
def make_groupings():
    rng = np.random.default_rng(91)
    frames = np.empty(N, np.uint32)                              # runs of 1 .. 40 consecutive rows, labelled by the run's first row
    far = np.empty(N, np.uint32)                                 # the same runs labelled by their LAST row: a run that crosses a cut carries
    lo = 0                                                       # a label of the next shard, and every label of shards 1 .. is >= 750
    while lo < N:
        hi = min(N, lo + int(rng.integers(1, 41)))
        frames[lo:hi], far[lo:hi] = lo, hi - 1
        lo = hi
    for cut in CUTS4[1:] + [375, 1125, 1875, 2625]:              # the premise: runs cross every cut of 4 and of 8 shards
        frames[cut - 1] = frames[cut] = frames[cut - 2]
        far[cut - 2:cut + 1] = far[cut]
    scattered = rng.integers(0, 300, N).astype(np.uint32)        # every group on every shard
    giant = np.full(N, NONE, np.uint32)
    giant[rng.choice(N, N * 9 // 10, replace=False)] = 5         # one group of 90 % of the rows, the rest ungrouped
    return {"frames": frames, "scattered": scattered, "giant": giant, "none": np.full(N, NONE, np.uint32), "short": frames[:1600].copy(),
            "far": far}


GROUPINGS = make_groupings()


def np_slice(labels, first, n_rows):
    """the canonical rule: a grouped row's label is the local id of the first row of its group inside the slice; NONE stays; as long as
    the part of the slice inside the grouping.  Returns (labels, count)."""
    part = labels[first:first + n_rows]
    out = np.full(len(part), NONE, np.uint32)
    first_of = {}
    for i, g in enumerate(part.tolist()):
        if g != NONE:
            out[i] = first_of.setdefault(g, i)
    return out, len(first_of) + int((part == NONE).sum())


def np_collapse(scores, ids, labels, k):
    """one row of records (any order, (LOWEST, NONE) = absent) -> the first k representatives by (score desc, id asc) under the grouping
    `labels` over global ids (an id at or past it, or of label NONE, is a group of its own), padded"""
    scores, ids = np.asarray(scores, np.int64).ravel(), np.asarray(ids, np.uint32).ravel()
    live = ids != NONE
    s, i = scores[live], ids[live]
    order = np.lexsort((i, ~s))
    s, i = s[order], i[order].astype(np.int64)
    lab = np.full(len(i), NONE, np.int64)
    inside = i < len(labels)
    lab[inside] = labels[i[inside]]
    key = np.where(lab == NONE, (1 << 32) + i, lab)              # an ungrouped record is its own group
    _, firsts = np.unique(key, return_index=True)
    keep = np.sort(firsts)[:k]
    out_s, out_i = np.full(k, LOWEST, np.int64), np.full(k, NONE, np.uint32)
    out_s[:len(keep)], out_i[:len(keep)] = s[keep], i[keep].astype(np.uint32)
    return out_s, out_i


def np_collapse_rows(scores, ids, labels, k):
    out = [np_collapse(s, i, labels, k) for s, i in zip(scores, ids)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- 1. slice against numpy ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def row_groups(gpu, mse):
    return {name: mse.RowGroups(g) for name, g in GROUPINGS.items()}


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 749, 750])
@pytest.mark.parametrize("first", [0, 1, 750, 2250])
def test_slice_equals_the_canonical_rule(row_groups, mse, first, n_rows):
    for name, labels in GROUPINGS.items():
        s = row_groups[name].slice(first, n_rows)
        want, count = np_slice(labels, first, n_rows)
        assert len(s) == len(want) == max(0, min(n_rows, len(labels) - first)), (name, first, n_rows)
        assert np.array_equal(s.to_host(), want), (name, first, n_rows)
        assert s.count == count, (name, first, n_rows)
        if first >= len(labels):                                   # wholly past the grouping: nothing to say
            assert len(s) == 0 and s.count == 0 and s.to_host().size == 0
        s.close()


def test_slice_on_the_named_device_round_trip_and_errors(row_groups, mse):
    s = row_groups["far"].slice(750, 750, device=0)
    want, count = np_slice(GROUPINGS["far"], 750, 750)
    assert np.array_equal(s.to_host(), want) and s.count == count
    assert (GROUPINGS["far"][750:1500] >= 750).all() and (want[want != NONE] < 750).all()    # labels past the shard's rows became local ids
    again = s.slice(0, 750)                                        # canonical labels are a fixed point
    assert np.array_equal(again.to_host(), want)
    for g in (s, again):
        g.close()
    assert np.array_equal(row_groups["scattered"].to_host(), GROUPINGS["scattered"])
    with pytest.raises(mse.MseError, match="n_rows"):
        row_groups["frames"].slice(0, 0)
    with pytest.raises(mse.MseError, match="device"):
        row_groups["frames"].slice(0, 10, device=99)
    from mse import ffi
    assert not ffi.lib().mse_groups_slice(None, 0, 10, -1) and "null" in ffi.last_error()
    assert ffi.lib().mse_groups_read(None, None) != 0 and "null" in ffi.last_error()


# ---- 2. the merge hook against numpy -------------------------------------------------------------------------------------------------
# The group table of the merge lives in LDS while a query has at most 4096 records (n_shards * k_in) and in global memory beyond:
# (8, 512) is the last LDS size, (8, 513) the first global one, (8, 1984) the largest exchange of 8 shards.
MERGE_SHAPES = [(4, 10), (8, 512), (8, 513), (8, 1984)]


def make_blocks(G, k_in, nq, seed):
    """hand-made records: shard s owns ids [s R, (s + 1) R); few distinct scores, so that ties within a group across shards and across
    groups are the rule; a tenth of the slots are holes, anywhere"""
    rng = np.random.default_rng(seed)
    R = 2 * k_in + 7
    scores = rng.integers(-20, 20, size=(G, nq, k_in)).astype(np.int64) * 1000
    ids = np.empty((G, nq, k_in), np.uint32)
    for s in range(G):
        for q in range(nq):
            ids[s, q] = s * R + rng.choice(R, k_in, replace=False)
    hole = rng.random((G, nq, k_in)) < 0.1
    scores[hole], ids[hole] = LOWEST, NONE
    return scores, ids, G * R


def pack(mse, scores, ids):
    from mse import ffi
    G, nq, k_in = scores.shape
    B = int(ffi.lib().mse_topk_block_bytes(nq, k_in))
    assert B % 16 == 0 and B >= nq * k_in * 12
    buf = np.zeros(G * B, np.uint8)
    for s in range(G):
        buf[s * B:s * B + nq * k_in * 8] = scores[s].ravel().view(np.uint8)
        buf[s * B + nq * k_in * 8:s * B + nq * k_in * 12] = ids[s].ravel().view(np.uint8)
    return buf, B


def unpack(buf, B, G, nq, k_in):
    scores = np.stack([buf[s * B:s * B + nq * k_in * 8].view(np.int64).reshape(nq, k_in) for s in range(G)])
    ids = np.stack([buf[s * B + nq * k_in * 8:s * B + nq * k_in * 12].view(np.uint32).reshape(nq, k_in) for s in range(G)])
    return scores, ids


@pytest.fixture(scope="module")
def scratch_searcher(gpu, mse, orc):
    vecs = mse.VectorList.from_f16s(orc.gen_rows_f16(SEED_BASE, 0, 64), D)
    return mse.Searcher(vecs)


# 70 queries at 15 872 records each: two launches over the global table (64 queries fit its 32 MiB)
MERGE_CASES = [(G, k_in, nq) for G, k_in in MERGE_SHAPES for nq in (1, 33)] + [(8, 1984, 70)]


@pytest.mark.parametrize("G,k_in,nq", MERGE_CASES)
def test_grouped_merge_equals_the_numpy_collapse(scratch_searcher, mse, G, k_in, nq):
    import torch
    from mse import ffi
    L = ffi.lib()
    scores, ids, n_ids = make_blocks(G, k_in, nq, 1000 * G + k_in + nq)
    rng = np.random.default_rng(k_in)
    g_len = n_ids - k_in                                             # the last shard's upper ids lie past the grouping
    assert (ids[ids != NONE] >= g_len).any()
    mixed = rng.integers(0, max(3, k_in // 2), g_len).astype(np.uint32)      # a group's records in every block
    mixed[rng.random(g_len) < 0.2] = NONE
    cases = {"mixed": mixed, "one": np.zeros(g_len, np.uint32), "none": np.full(g_len, NONE, np.uint32)}
    for name, labels in cases.items():
        rg = mse.RowGroups(labels)
        for k in sorted({1, K, min(k_in, 200)}):
            buf, B = pack(mse, scores, ids)
            dev = torch.from_numpy(buf).cuda()
            out_s = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            out_i = torch.empty((nq, k), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ffi.check(L.mse_merge_topk_packed_grouped_dev(scratch_searcher._h, rg._h, dev.data_ptr(), G, nq, k_in, k, out_s.data_ptr(),
                                                          out_i.data_ptr()), "merge_topk_packed_grouped")
            ffi.check(L.mse_device_synchronize(), "sync")
            got_s, got_i = out_s.cpu().numpy(), out_i.cpu().numpy().view(np.uint32)
            flat_s = scores.transpose(1, 0, 2).reshape(nq, G * k_in)
            flat_i = ids.transpose(1, 0, 2).reshape(nq, G * k_in)
            want_s, want_i = np_collapse_rows(flat_s, flat_i, labels, k)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, k)
            if name == "one":                                         # every grouped record in one group: it and the ungrouped tail
                grouped = (want_i < g_len).sum(axis=1)
                assert (grouped <= 1).all()
            if name == "none" and k_in == k:                          # all NONE: the plain merge, and the blocks are left as they were
                ffi.check(L.mse_merge_topk_packed_dev(scratch_searcher._h, dev.data_ptr(), G, nq, k, out_s.data_ptr(), out_i.data_ptr()), "merge")
                ffi.check(L.mse_device_synchronize(), "sync")
                assert np.array_equal(out_s.cpu().numpy(), got_s) and np.array_equal(out_i.cpu().numpy().view(np.uint32), got_i)
                assert np.array_equal(dev.cpu().numpy(), buf)
            # in place: exactly the non-representatives of a group became holes
            after_s, after_i = unpack(dev.cpu().numpy(), B, G, nq, k_in)
            all_s, all_i = np_collapse_rows(flat_s, flat_i, labels, G * k_in)
            for q in range(nq):
                kept = set(all_i[q][all_i[q] != NONE].tolist())
                stay = np.isin(ids[:, q], list(kept)) & (ids[:, q] != NONE)
                assert np.array_equal(after_i[:, q], np.where(stay, ids[:, q], NONE)), (name, k, q)
                assert np.array_equal(after_s[:, q], np.where(stay, scores[:, q], LOWEST)), (name, k, q)
        rg.close()


def test_grouped_merge_ties_and_errors(scratch_searcher, mse):
    import torch
    from mse import ffi
    L = ffi.lib()
    # two shards, one query: group 0 = ids {3, 40} with equal scores in different shards (the lower id wins), groups 1 and 2 tie with
    # each other (the lower id first), a hole in the middle of block 0, id 99 past the grouping
    scores = np.array([[[500, LOWEST, 500, 100]], [[500, 500, 700, 100]]], np.int64)
    ids = np.array([[[40, NONE, 7, 99]], [[3, 50, 41, 60]]], np.uint32)
    labels = np.full(64, NONE, np.uint32)
    labels[[3, 40]] = 0                                                # (41 stays ungrouped)
    labels[7], labels[50], labels[60] = 1, 2, 1
    rg = mse.RowGroups(labels)
    buf, B = pack(mse, scores, ids)
    dev = torch.from_numpy(buf).cuda()
    out_s = torch.empty((1, 6), dtype=torch.int64, device="cuda")
    out_i = torch.empty((1, 6), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ffi.check(L.mse_merge_topk_packed_grouped_dev(scratch_searcher._h, rg._h, dev.data_ptr(), 2, 1, 4, 6, out_s.data_ptr(), out_i.data_ptr()), "merge")
    ffi.check(L.mse_device_synchronize(), "sync")
    assert out_i.cpu().numpy().view(np.uint32).tolist() == [[41, 3, 7, 50, 99, NONE]]
    assert out_s.cpu().numpy().tolist() == [[700, 500, 500, 500, 100, LOWEST]]
    assert L.mse_merge_topk_packed_grouped_dev(scratch_searcher._h, None, dev.data_ptr(), 2, 1, 4, 6, out_s.data_ptr(), out_i.data_ptr()) != 0
    assert "null grouping" in ffi.last_error()
    assert L.mse_merge_topk_packed_grouped_dev(None, rg._h, dev.data_ptr(), 2, 1, 4, 6, out_s.data_ptr(), out_i.data_ptr()) != 0
    assert "null searcher" in ffi.last_error()
    rg.close()


# ---- 3. brute force -----------------------------------------------------------------------------------------------------------------
NQS, KS = (1, 7, 320), (1, 10, 200)


@pytest.fixture(scope="module")
def flat(gpu, mse, orc):
    """the unsharded side, made once: rows, queries, the searcher over all rows, the oracle's full ranking of the first 7 queries and a
    cache of the unsharded grouped answers, shared by every group size"""
    base = orc.gen_rows_f16(SEED_BASE, 0, N)
    q = orc.gen_rows_f16(SEED_QUERY, 0, 320)
    vecs = mse.VectorList.from_f16s(base, D)
    rank_s, rank_i = orc.bruteforce_topk(base, q[:7], N)
    half = group_masks(N, 4, mse)["half"]
    return {"base": base, "q": q, "whole": mse.Searcher(vecs), "rank": (rank_s, rank_i.astype(np.uint32)), "half": half, "rf": mse.RowFilter(half),
            "cache": {}}


def unsharded(flat, mse, row_groups, name, nq, k, mode, filtered):
    key = (name, nq, k, mode, filtered)
    if key not in flat["cache"]:
        flat["cache"][key] = flat["whole"].bruteforce_topk(flat["q"][:nq], k, mode, allow=flat["rf"] if filtered else None, groups=row_groups[name])
    return flat["cache"][key]


@pytest.mark.parametrize("name", list(GROUPINGS))
@pytest.mark.parametrize("G", [1, 4, 8])
def test_sharded_grouped_bruteforce_equals_the_unsharded_call_and_the_oracle(flat, row_groups, mse, G, name):
    grp = mse.ShardGroup(G, D, devices=[0] * G)
    grp.load_host(flat["base"])
    if G == 4:
        assert [grp.first_row(g) for g in range(G)] == CUTS4
    labels = GROUPINGS[name]
    sg = grp.groups(row_groups[name])
    assert sg.n_shards == G
    for g in range(G):
        lo, hi = mse.shard_range(N, g, G)
        part = sg.shard(g)
        if lo >= len(labels):
            assert part is None                                        # wholly past the grouping ("short": shard 3 of 4)
        else:
            want, count = np_slice(labels, lo, hi - lo)
            assert np.array_equal(part.to_host(), want) and part.count == count, (name, g)
    if name == "short" and G == 4:
        assert sg.shard(3) is None and len(sg.shard(2)) == 100
    sf = grp.filter(flat["rf"])
    rank_s, rank_i = flat["rank"]
    dense = 0
    for filtered in (False, True):
        for nq in NQS:
            for k in KS:
                for mode in (mse.MODE_AUTO, mse.MODE_EXACT):
                    us, ui = unsharded(flat, mse, row_groups, name, nq, k, mode, filtered)
                    gs, gi = grp.bruteforce_topk_grouped(sg, flat["q"][:nq], k, sf if filtered else None, mode)
                    assert np.array_equal(gi, ui) and np.array_equal(gs, us), (name, filtered, nq, k, mode)
                    if mode == mse.MODE_AUTO:
                        dense += sum(grp.searcher(g).grouped_stats()[2] for g in range(G) if sg.shard(g) is not None)
                    if nq <= 7:                                        # the collapse of the oracle's full ranking
                        for q in range(nq):
                            ok = flat["half"][rank_i[q]] if filtered else np.ones(N, bool)
                            ws, wi = np_collapse(rank_s[q][ok], rank_i[q][ok], labels, k)
                            assert np.array_equal(gi[q], wi) and np.array_equal(gs[q], ws), (name, filtered, nq, k, mode, q)
                    if name == "none" and not filtered:
                        ps, pi = grp.bruteforce_topk(flat["q"][:nq], k, mode)
                        assert np.array_equal(gi, pi) and np.array_equal(gs, ps), (nq, k, mode)
    if name == "giant":
        assert dense > 0, "a shard whose rows are one group and a few ungrouped ones cannot fill k = 200 from a prefix"
    sf.close()
    sg.close()
    grp.close()


def test_sharded_grouped_bruteforce_device_form_and_mfma(flat, row_groups, mse):
    import torch
    grp = mse.ShardGroup(4, D, devices=[0] * 4)
    grp.load_host(flat["base"])
    sg = grp.groups(row_groups["scattered"])
    nq = 7
    qd = torch.from_numpy(flat["q"][:nq].view(np.int16)).cuda()
    out_s = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    out_i = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for mode in (mse.MODE_MFMA, mse.MODE_AUTO, mse.MODE_EXACT):
        grp.bruteforce_topk_grouped_dev(sg, qd.data_ptr(), nq, K, out_s.data_ptr(), out_i.data_ptr(), mode=mode)
        us, ui = flat["whole"].bruteforce_topk(flat["q"][:nq], K, mode, groups=row_groups["scattered"])
        assert np.array_equal(out_s.cpu().numpy(), us) and np.array_equal(out_i.cpu().numpy().view(np.uint32), ui), mode
        gs, gi = grp.bruteforce_topk_grouped(sg, flat["q"][:nq], K, None, mode)
        assert np.array_equal(gs, us) and np.array_equal(gi, ui), mode
    sg.close()
    grp.close()


# ---- 4. graph and 5. PQ scan: one small index per group size ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anns(gpu, mse, orc):
    made = {}

    def get(G):
        if G not in made:
            a = Ann(mse, orc, G, 170 + G)
            a.luts = np.stack([a.pq.preprocess_query(q).table.reshape(-1) for q in orc.f16_to_f32(a.qh)])
            made[G] = a
        return made[G]
    return get


GRAPH_GROUPINGS = ("frames", "scattered", "giant", "short", "far")
K_ALL = 1984            # the largest k: a merged ungrouped answer of this size holds everything the shards visited (asserted)


@pytest.mark.parametrize("disable_pq", [True, False])
@pytest.mark.parametrize("G", [1, 4, 8])
def test_sharded_grouped_graph_query_is_the_collapse_of_what_the_shards_visited(anns, row_groups, mse, G, disable_pq):
    a = anns(G)
    luts = None if disable_pq else a.luts
    for L in (16, 64):
        all_s, all_i = a.grp.query_topk(a.qh, K_ALL, luts, None, disable_pq, 4, L)
        assert (all_i[:, -1] == NONE).all() and (all_i[:, 0] != NONE).all(), "the reference must hold every visited record"
        for name in GRAPH_GROUPINGS:
            sg = a.grp.groups(row_groups[name])
            got_s, got_i = a.grp.query_topk_grouped(sg, a.qh, K, luts, None, disable_pq, 4, L)
            want_s, want_i = np_collapse_rows(all_s, all_i, GROUPINGS[name], K)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, L)
            if name == "giant" and L == 16 and G == 1:                # a search list of 16 visits a few dozen rows, nine tenths of them
                assert (got_i[:, -1] == NONE).all() and (got_i[:, 0] != NONE).all()       # one group: short, and padded
            sg.close()


@pytest.mark.parametrize("G", [1, 4])
def test_sharded_grouped_graph_query_under_a_shard_filter(anns, row_groups, mse, G):
    a = anns(G)
    mask = group_masks(N, G, mse)["half"]
    rf = mse.RowFilter(mask)
    sf = a.grp.filter(rf)
    sc_q = np.ascontiguousarray(np.broadcast_to(SCALES, (len(a.qh), 4)))
    for regime in ("graph", "list"):
        for L in (16, 64):
            for sc in (None, sc_q):
                all_s, all_i = a.grp.query_topk_filtered(sf, a.qh, K_ALL, None, sc, True, 4, L, regime)
                assert (all_i[:, -1] == NONE).all()
                assert mask[all_i[all_i != NONE]].all()
                for name in ("frames", "scattered", "short"):
                    sg = a.grp.groups(row_groups[name])
                    got_s, got_i = a.grp.query_topk_grouped(sg, a.qh, K, None, sc, True, 4, L, sf, regime)
                    want_s, want_i = np_collapse_rows(all_s, all_i, GROUPINGS[name], K)
                    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, regime, L, sc is not None)
                    sg.close()
    sf.close()
    rf.close()


@pytest.mark.parametrize("G", [1, 4, 8])
def test_sharded_grouped_pq_scan_is_the_collapse_of_the_reranked_top_r(anns, row_groups, mse, G):
    a = anns(G)
    mask = group_masks(N, G, mse)["half"]
    rf = mse.RowFilter(mask)
    sf = a.grp.filter(rf)
    for r in (50, 200):
        for sc in (None, SCALES):
            all_s, all_i = a.grp.pq_scan_topk(a.qs, r, r, sc)
            fil_s, fil_i = a.grp.pq_scan_topk_filtered(sf, a.qs, r, r, sc)
            for name in GRAPH_GROUPINGS + ("none",):
                sg = a.grp.groups(row_groups[name])
                got_s, got_i = a.grp.pq_scan_topk_grouped(sg, a.qs, r, K, sc)
                want_s, want_i = np_collapse_rows(all_s, all_i, GROUPINGS[name], K)
                assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, r, sc is not None)
                if name == "giant":                                    # 50 candidates hold about 5 ungrouped rows and the one group
                    assert r == 200 or (got_i[:, -1] == NONE).any()
                if name == "none":
                    ps, pi = a.grp.pq_scan_topk(a.qs, r, K, sc)
                    assert np.array_equal(got_i, pi) and np.array_equal(got_s, ps)
                for mode in ("scan", "list"):
                    got_s, got_i = a.grp.pq_scan_topk_grouped(sg, a.qs, r, K, sc, sf, mode)
                    want_s, want_i = np_collapse_rows(fil_s, fil_i, GROUPINGS[name], K)
                    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), (name, r, sc is not None, mode)
                sg.close()
    sf.close()
    rf.close()


# ---- 6. lifetime and errors ---------------------------------------------------------------------------------------------------------
def test_stale_foreign_and_null_shard_groups_are_refused_without_writing(anns, flat, row_groups, mse):
    from mse import ffi
    from mse.vector import _p
    a = anns(4)
    L = ffi.lib()
    rg = mse.RowGroups(GROUPINGS["scattered"])
    other = mse.ShardGroup(4, D, devices=[0] * 4)
    other.load_host(flat["base"])
    foreign = other.groups(rg)
    stale = a.grp.groups(rg)
    rf = mse.RowFilter(group_masks(N, 4, mse)["half"])
    stale_sf = a.grp.filter(rf)
    good_before = a.grp.bruteforce_topk_grouped(stale, a.qh, K)
    nq = len(a.qh)

    def calls(grp, sg, sf, s0, i0, nq=nq, k=K):
        return [
            lambda: L.mse_shard_group_search_grouped(grp._h, sg, sf, _p(a.qh, C.c_uint16), nq, k, 0, _p(s0, C.c_int64), _p(i0, C.c_uint32)),
            lambda: L.mse_shard_group_pq_scan_topk_grouped(grp._h, sg, sf, _p(a.qs, C.c_float), None, nq, 64, k, 0, _p(s0, C.c_int64),
                                                           _p(i0, C.c_uint32)),
            lambda: L.mse_shard_group_query_topk_grouped(grp._h, sg, sf, _p(a.qh, C.c_uint16), None, None, nq, 1, 2, 24, k, 0, _p(s0, C.c_int64),
                                                         _p(i0, C.c_uint32)),
        ]

    def refused(grp, sg, sf, match):
        s0, i0 = np.full((nq, K), 12345, np.int64), np.full((nq, K), 54321, np.uint32)
        for call in calls(grp, sg, sf, s0, i0):
            assert call() != 0
            assert match in ffi.last_error(), ffi.last_error()
            assert (s0 == 12345).all() and (i0 == 54321).all()

    refused(a.grp, foreign._h, None, "another group")
    refused(a.grp, None, None, "null shard groups")
    refused(a.grp, None, stale_sf._h, "null shard groups")
    with pytest.raises(TypeError):
        a.grp.bruteforce_topk_grouped(rg, a.qh, K)                     # a RowGroups is not a ShardGroups
    longer = mse.RowGroups(np.zeros(N + 1, np.uint32))
    with pytest.raises(mse.MseError, match="longer"):
        a.grp.groups(longer)
    longer.close()
    # nothing to do: 0, and nothing is written
    s0, i0 = np.full((nq, K), 12345, np.int64), np.full((nq, K), 54321, np.uint32)
    for call in calls(a.grp, stale._h, None, s0, i0, nq=0) + calls(a.grp, stale._h, None, s0, i0, k=0):
        assert call() == 0
        assert (s0 == 12345).all() and (i0 == 54321).all()
    # the same rows loaded again: a new layout.  The filter's check comes first; a null sg is named after it
    a.grp.load_host(a.base)
    refused(a.grp, stale._h, None, "before the group's rows were replaced")
    refused(a.grp, None, stale_sf._h, "shard filter was made for another group")
    fresh_sf = a.grp.filter(rf)
    refused(a.grp, stale._h, fresh_sf._h, "shard groups were made for another group")
    fresh = a.grp.groups(rg)
    got = a.grp.bruteforce_topk_grouped(fresh, a.qh, K)
    assert np.array_equal(got[0], good_before[0]) and np.array_equal(got[1], good_before[1])
    # closing the caller's RowGroups: the shard groups still answer; closing the shard groups: the RowGroups is still usable
    rg2 = mse.RowGroups(GROUPINGS["scattered"])
    sg2 = a.grp.groups(rg2)
    rg2.close()
    got = a.grp.bruteforce_topk_grouped(sg2, a.qh, K)
    assert np.array_equal(got[0], good_before[0]) and np.array_equal(got[1], good_before[1])
    sg2.close()
    fresh.close()
    us, ui = a.whole.bruteforce_topk(a.qh, K, groups=rg)
    assert np.array_equal(us, good_before[0]) and np.array_equal(ui, good_before[1])
    for x in (foreign, stale, stale_sf, fresh_sf, rf, rg):
        x.close()
    other.close()


# ---- 7. handle reuse ----------------------------------------------------------------------------------------------------------------
def test_alternating_grouped_ungrouped_and_filtered_calls_repeat_their_first_answers(anns, flat, row_groups, mse):
    a = anns(4)
    rf = mse.RowFilter(group_masks(N, 4, mse)["half"])
    sf = a.grp.filter(rf)
    sgs = {name: a.grp.groups(row_groups[name]) for name in ("frames", "giant")}
    qh320 = np.concatenate([a.qh] * 36)[:320]
    calls = {
        "bf_grouped_9_10": lambda: a.grp.bruteforce_topk_grouped(sgs["frames"], a.qh, 10),
        "bf_plain_1_200": lambda: a.grp.bruteforce_topk(a.qh[:1], 200),
        "bf_grouped_320_1": lambda: a.grp.bruteforce_topk_grouped(sgs["giant"], qh320, 1, None, mse.MODE_EXACT),
        "bf_filtered_9_10": lambda: a.grp.bruteforce_topk_filtered(sf, a.qh, 10),
        "bf_grouped_filtered_3_200": lambda: a.grp.bruteforce_topk_grouped(sgs["giant"], a.qh[:3], 200, sf),
        "graph_grouped_9_10": lambda: a.grp.query_topk_grouped(sgs["frames"], a.qh, 10, None, None, True, 4, 64),
        "graph_plain_9_1984": lambda: a.grp.query_topk(a.qh, K_ALL, None, None, True, 4, 64),
        "graph_grouped_2_1984": lambda: a.grp.query_topk_grouped(sgs["giant"], a.qh[:2], K_ALL, None, None, True, 4, 16),
        "graph_filtered_9_10": lambda: a.grp.query_topk_filtered(sf, a.qh, 10, None, None, True, 4, 64, "graph"),
        "pq_grouped_9_200_10": lambda: a.grp.pq_scan_topk_grouped(sgs["frames"], a.qs, 200, 10, SCALES),
        "pq_plain_1_50": lambda: a.grp.pq_scan_topk(a.qs[:1], 50, 50),
        "pq_grouped_filtered_9_50_10": lambda: a.grp.pq_scan_topk_grouped(sgs["giant"], a.qs, 50, 10, None, sf, "scan"),
    }
    first = {name: call() for name, call in calls.items()}
    rng = np.random.default_rng(93)
    names = list(calls)
    for _ in range(3):
        for j in rng.permutation(len(names)):
            s, i = calls[names[j]]()
            assert np.array_equal(s, first[names[j]][0]) and np.array_equal(i, first[names[j]][1]), names[j]
    for x in list(sgs.values()) + [sf, rf]:
        x.close()
