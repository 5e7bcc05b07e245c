"""The OPQ/PQ flat scan over an allowed-row set (mse_pq_scan_topk*_filtered) and the live-row filter of a mutated graph
(mse_graph_live_filter).  The rule under test: a filtered call returns exactly what the unfiltered call returns on codes (and base rows)
made of the allowed rows alone, ids mapped back -- so every expected value is the CPU oracle applied to codes[allowed]."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_pq
from test_gpu_filtered_graph import clustered_rows, knn_graph
from test_gpu_graph_delete import cfgs

pytestmark = pytest.mark.gpu
D = 1152
NONE = 0xFFFFFFFF
I64_MIN = np.iinfo(np.int64).min
MODES = ("scan", "list")


def oracle_topk(orc, opq, lut, codes, bias, allowed, r, k, base=None, qh=None):
    """The unfiltered pipeline on the allowed rows alone (ascending ids), ids mapped back, padded to k.  bias: the descriptor product of
    every row (or None); base + qh: the fp16 re-score of the r best."""
    allowed = np.asarray(allowed, np.int64)
    out_s, out_i = np.full(k, I64_MIN, np.int64), np.full(k, NONE, np.uint32)
    if allowed.size == 0:
        return out_s, out_i
    approx = opq.asymmetric_dot_product(lut, codes[allowed])
    if bias is not None:
        approx = approx + bias[allowed]
    if base is None:
        ws, wi = orc.topk_from_scores(approx, min(k, allowed.size))
    else:
        _, cand = orc.topk_from_scores(approx, min(r, allowed.size))
        exact = orc.score_rows(base[allowed], cand, qh)
        if bias is not None:
            exact = exact + bias[allowed][cand]
        order = np.lexsort((cand, -exact))[:k]
        ws, wi = exact[order], cand[order]
    out_s[:len(wi)], out_i[:len(wi)] = ws, allowed[wi]
    return out_s, out_i


def descriptor_bias(opq, codes, desc, scales):
    """descriptor_product of every row through the oracle: its ADC with an all-zero table is the bias alone"""
    return opq.adc_desc(np.zeros((64, 256), np.float32), codes, desc, scales)


def filters_for(n, r, k, rng):
    """name -> boolean mask; its length is the filter's length (one of them is shorter than the codes)"""
    def pick(count):
        m = np.zeros(n, bool)
        m[rng.choice(n, count, replace=False)] = True
        return m
    g = np.arange(n) // 64
    short = max(n - 37, 0)
    return {
        "all rows": np.ones(n, bool),
        "none": np.zeros(n, bool),
        "one row": pick(1),
        "every other row": np.arange(n) % 2 == 1,
        "one whole group excluded": g != (1 if n > 64 else 0),
        "only the last partial group": g == (n - 1) // 64,
        "only group 0": g == 0,
        "random 1 %": rng.random(n) < 0.01,
        "random 50 %": rng.random(n) < 0.5,
        "37 rows shorter than the codes": rng.random(short) < 0.7,
        "a count below k": pick(max(min(n, k) - 1, 0)),
        "a count below r": pick(max(min(n, r) - 1, 0)),
    }


@pytest.mark.parametrize("n,r,k", [(70, 200, 10), (4097, 64, 64), (12345, 200, 10), (64, 5, 5), (1, 3, 2)])
def test_subset_identity_ragged_and_tied(gpu, mse, orc, n, r, k):
    """Seven distinct code rows and descriptors in 0..2 (id order decides almost everything), five queries per batch (two pairs and a
    single), twelve filters; each with and without descriptors, with and without the fp16 re-score, in SCAN and LIST: all equal the
    oracle on codes[allowed] and each other bit for bit, the batch equals one-by-one calls, the all-rows filter the unfiltered call."""
    rng = np.random.default_rng(n)
    cents, T, _, _ = make_pq(orc)
    opq, gpq = orc.PQ(cents, T, 18, D), mse.ProductQuantizer(cents, T, 18, D)
    distinct = rng.integers(0, 256, size=(7, 64), dtype=np.uint8)
    codes = distinct[rng.integers(0, 7, size=n)]
    desc = rng.integers(0, 3, size=(n, 4), dtype=np.uint8)
    scales = np.array([0.25, 0, -0.125, 0.5], np.float32) / np.float32(512)
    base = orc.f16_bits((rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32))
    searcher = mse.Searcher(mse.VectorList.from_f16s(base, D))
    qs = (rng.standard_normal((5, D)) / np.sqrt(D)).astype(np.float32)
    luts = [opq.preprocess_query(q) for q in qs]
    qhs = [orc.f16_bits(q) for q in qs]
    bias = descriptor_bias(opq, codes, desc, scales)
    variants = [(mse.Codes(codes, desc), scales, bias), (mse.Codes(codes, None), None, None)]
    for name, mask in filters_for(n, r, k, rng).items():
        allowed = np.flatnonzero(mask)
        f = mse.RowFilter(mask)
        assert len(f) == mask.size and f.count == allowed.size
        for gcodes, sc, bs in variants:
            for s in (None, searcher):
                want = [oracle_topk(orc, opq, luts[j], codes, bs, allowed, r, k, base if s else None, qhs[j]) for j in range(5)]
                for mode in MODES:
                    got_s, got_i = gpq.scan_topk_batch_filtered(gcodes, f, qs, r, k, s, sc, mode)
                    for j in range(5):
                        tag = (name, sc is not None, s is not None, mode, j)
                        assert np.array_equal(got_i[j], want[j][1]) and np.array_equal(got_s[j], want[j][0]), tag
                        s1, i1 = gpq.scan_topk_filtered(gcodes, f, qs[j], r, k, s, sc, mode)
                        assert np.array_equal(s1, got_s[j]) and np.array_equal(i1, got_i[j]), tag
                if name == "all rows":
                    us, ui = gpq.scan_topk_batch(gcodes, qs, r, k, s, sc)
                    assert np.array_equal(us, np.stack([w[0] for w in want])) and np.array_equal(ui, np.stack([w[1] for w in want]))
        f.close()


@pytest.mark.parametrize("n", [70, 4097])
@pytest.mark.parametrize("codec", ["64 x 256, three descriptors", "8 x 8"])
def test_full_score_route(gpu, mse, orc, codec, n):
    """The codec shapes without a group-maximum scan -- 64 x 256 with three descriptor bytes per row, and 8 chunks x 8 centroids --
    score every row (unfiltered) or the filter's id list (either mode).  Five queries per batch (two pairs and a single): the batch
    and the one-by-one calls equal the oracle pipeline bit for bit, and the all-rows filter equals the unfiltered call."""
    r, k = 64, 10
    rng = np.random.default_rng(n)
    if codec == "8 x 8":
        d, dpc, nc = 128, 16, 8
        desc = scales = None
    else:
        d, dpc, nc = D, 18, 256
        desc = rng.integers(0, 3, size=(n, 3), dtype=np.uint8)
        scales = np.array([0.25, -0.125, 0.5], np.float32) / np.float32(512)
    cents, T, _, _ = make_pq(orc, d, dpc, nc)
    opq, gpq = orc.PQ(cents, T, dpc, d), mse.ProductQuantizer(cents, T, dpc, d)
    codes = rng.integers(0, nc, size=(n, d // dpc), dtype=np.uint8)
    gcodes = mse.Codes(codes, desc)
    qs = (rng.standard_normal((5, d)) / np.sqrt(d)).astype(np.float32)
    luts = [opq.preprocess_query(q) for q in qs]
    bias = None if desc is None else opq.adc_desc(np.zeros((d // dpc, nc), np.float32), codes, desc, scales)
    searchers = [None]
    base = qhs = None
    if d == D:   # (the re-score at the width it is tested at)
        base = orc.f16_bits((rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32))
        qhs = [orc.f16_bits(q) for q in qs]
        searchers.append(mse.Searcher(mse.VectorList.from_f16s(base, D)))
    masks = filters_for(n, r, k, rng)
    for s in searchers:
        def want_for(allowed):
            return [oracle_topk(orc, opq, luts[j], codes, bias, allowed, r, k, base if s else None, qhs[j] if s else None) for j in range(5)]
        want = want_for(np.arange(n))
        us, ui = gpq.scan_topk_batch(gcodes, qs, r, k, s, scales)
        for j in range(5):
            tag = (s is not None, j)
            assert np.array_equal(ui[j], want[j][1]) and np.array_equal(us[j], want[j][0]), tag
            s1, i1 = gpq.scan_topk(gcodes, qs[j], r, k, s, scales)
            assert np.array_equal(s1, us[j]) and np.array_equal(i1, ui[j]), tag
        for name in ("random 50 %", "a count below r", "none", "all rows"):
            f = mse.RowFilter(masks[name])
            want = want_for(np.flatnonzero(masks[name]))
            for mode in MODES:
                got_s, got_i = gpq.scan_topk_batch_filtered(gcodes, f, qs, r, k, s, scales, mode)
                for j in range(5):
                    tag = (name, s is not None, mode, j)
                    assert np.array_equal(got_i[j], want[j][1]) and np.array_equal(got_s[j], want[j][0]), tag
                    s1, i1 = gpq.scan_topk_filtered(gcodes, f, qs[j], r, k, s, scales, mode)
                    assert np.array_equal(s1, got_s[j]) and np.array_equal(i1, got_i[j]), tag
                if name == "all rows":
                    assert np.array_equal(got_s, us) and np.array_equal(got_i, ui), (s is not None, mode)
            f.close()


def group_filters(n, rng):
    """random 50 %, random 1/64 and a filter shorter than the codes, each with some groups fully excluded"""
    g = np.arange(n) // 64
    empty = np.isin(g, [0, 3, 17, 18, (n - 1) // 64])
    short = n - 64 * 5 - 21
    out = {"random 50 %": (rng.random(n) < 0.5) & ~empty, "random 1/64": (rng.random(n) < 1 / 64) & ~np.isin(g, [3, 17])}
    out["shorter than the codes"] = ((rng.random(n) < 0.6) & ~empty)[:short]
    return out


@pytest.mark.parametrize("n", [64 * 300, 64 * 97 + 13])
def test_masked_group_maxima_one_and_two_queries(gpu, mse, orc, n):
    """pq_scan64_kernel<true, true> and pq_scan64x2_kernel<.., true>: every group maximum equals the maximum of the gather kernel's
    scores over the group's ALLOWED vectors (the same i64, which the select's floor leans on), INT64_MIN for a group without one."""
    rng = np.random.default_rng(n)
    cents, T, _, _ = make_pq(orc)
    gpq = mse.ProductQuantizer(cents, T, 18, D)
    codes = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    gcodes = mse.Codes(codes, desc)
    luts = [(rng.standard_normal(64 * 256) * 10.0 ** rng.uniform(-4, 1, size=64 * 256)).astype(np.float32) for _ in range(2)]
    ids = np.arange(n, dtype=np.uint32)
    ng = (n + 63) // 64
    for scales in (None, np.array([0.5, -0.25, 3.0, 1e-3], np.float32) / np.float32(512)):
        gathered = [gpq.adc_gather(gcodes, lut, ids, scales) for lut in luts]
        for name, mask in group_filters(n, rng).items():
            full = np.zeros(ng * 64, bool)
            full[:mask.size] = mask
            f = mse.RowFilter(mask)
            one = [gpq.debug_group_max_filtered(gcodes, f, lut, None, scales) for lut in luts]
            two = gpq.debug_group_max_filtered(gcodes, f, luts[0], luts[1], scales)
            for j in range(2):
                pad = np.full(ng * 64, I64_MIN, np.int64)
                pad[:n] = gathered[j]
                pad[~full] = I64_MIN
                want = pad.reshape(ng, 64).max(axis=1)
                assert (want == I64_MIN).sum() >= 2                         # some groups are empty
                assert np.array_equal(one[j], want) and np.array_equal(two[j], want), (name, j, scales is None)
            f.close()


def integer_tables(lut, scales, per_pass):
    """The nomination scan's tables restated (pq4_quant_kernel): (delta, c, entries [64][256], descriptor entries [4][256] or None)"""
    code_max, desc_max = (4095.0, 16383.0) if per_pass == 4 else (255.0, 16383.0)
    lut = lut.reshape(64, 256).astype(np.float64)
    lo, hi = lut.min(axis=1), lut.max(axis=1)
    delta = (hi - lo).max() / code_max
    c_sum = 0.0
    for c in range(64):
        c_sum += lo[c]
    if scales is not None:
        for sc in scales.astype(np.float64):
            delta = max(delta, abs(sc) * 255.0 / desc_max)
            c_sum += min(0.0, sc * 255.0)
    delta = max(delta, 1e-300)
    inv = 1.0 / delta
    e = np.clip(np.rint((lut - lo[:, None]) * inv), 0, code_max).astype(np.int32)
    ed = None
    if scales is not None:
        ed = np.stack([np.clip(np.rint((sc * np.arange(256.0) - min(0.0, sc * 255.0)) * inv), 0, desc_max).astype(np.int32)
                       for sc in scales.astype(np.float64)])
    return delta, c_sum, e, ed


def integer_sums(e, ed, codes, desc):
    s = e[np.arange(64)[None, :], codes].sum(axis=1, dtype=np.int64)
    if ed is not None:
        for dd in range(4):
            s = s + ed[dd][desc[:, dd]]
    return s


@pytest.mark.parametrize("n,per_pass", [(64 * 300, 4), (64 * 97 + 13, 4), (64 * 300, 8), (64 * 97 + 13, 8)])
def test_masked_group_maxima_four_and_eight_queries(gpu, mse, orc, n, per_pass):
    """pq_scan64x4_kernel<.., 4, true> and <.., 8, true>: every group maximum equals the maximum of the integer sums -- restated from the
    tables' own parameters, as test_pq4_matrix_core_scan_equals_integer_sums restates them -- over the group's allowed vectors; a group
    without one gives the zero-sum key."""
    rng = np.random.default_rng(n + per_pass)
    cents, T, _, _ = make_pq(orc)
    gpq = mse.ProductQuantizer(cents, T, 18, D)
    codes = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    desc = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    gcodes = mse.Codes(codes, desc)
    luts = (rng.standard_normal((per_pass, 64, 256)) * rng.uniform(0.01, 0.3, (per_pass, 64, 1))).astype(np.float32)
    ng = (n + 63) // 64
    for scales in (np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512), None):
        sums = []
        for j in range(per_pass):
            delta, c_sum, e, ed = integer_tables(luts[j], scales, per_pass)
            sums.append((delta, c_sum, integer_sums(e, ed, codes, desc)))
        for name, mask in group_filters(n, rng).items():
            full = np.zeros(ng * 64, bool)
            full[:mask.size] = mask
            out, params = gpq.debug_group_max4_filtered(gcodes, mask, luts, scales, per_pass=per_pass)
            for j in range(per_pass):
                delta, c_sum, s = sums[j]
                assert params[j, 0] == delta and params[j, 1] == c_sum and params[j, 3] == 1
                pad = np.zeros(ng * 64, np.int64)
                pad[:n] = s
                pad[~full] = 0
                want = pad.reshape(ng, 64).max(axis=1)
                assert (want == 0).sum() >= 2
                assert np.array_equal(out[j].astype(np.int64), want), (name, j, scales is None, np.flatnonzero(out[j] != want)[:5])


def certificate_margin(maxima, delta, c_sum, eps, approx_allowed, groups_allowed, r, per_pass):
    """The certificate of pq4_certify_kernel restated for one query: nominate the n_nom best groups by (masked integer maximum desc,
    group asc); the r-th best reference-order score among the allowed vectors of those groups, minus the bound on everything outside
    them (the best excluded group's key), in score units of 2^-32.  Positive = the query is certified."""
    n_nom = r + max(64, r // 2) if per_pass == 4 else 2 * r + 112
    order = np.lexsort((np.arange(maxima.size), -maxima.astype(np.int64)))
    nominated = np.zeros(maxima.size, bool)
    nominated[order[:n_nom]] = True
    inside = np.sort(approx_allowed[nominated[groups_allowed]])[::-1]
    assert inside.size >= r
    ub = (delta * float(maxima[order[n_nom]]) + c_sum + eps) * 4294967296.0
    return float(inside[r - 1]) - ub


def test_four_and_eight_per_pass_filtered(gpu, mse, orc):
    """300 000 random codes, r = 120, k = 10, batches of 9 (eight per pass + a single), 8 (eight per pass) and 4 (four per pass) queries
    under the all-rows, a random 50 % and a random 1/64 filter: the oracle's answers in every case.  All-rows and 50 % must also be
    CERTIFIED (last_uncertified == 0: the masked nomination scan really answers), which for the 50 % filter is first shown to be what the
    certificate itself says, restated on the host from the hook's parameters and masked maxima -- seed 91, smallest margin over the
    twelve (query, tables) pairs checked: 2.1e7 score units of 2^-32 (0.005 as a dot product; the test prints them).  No bound is asserted for the 1/64 filter (fewer than r allowed vectors may
    lie in the nominated groups), only exact answers.  On seven distinct code rows every query is uncertified and still exact.
    Filtered batches never switch the handle to four per pass: the last unfiltered batch of eight is still certified."""
    rng = np.random.default_rng(91)
    cents, T, _, _ = make_pq(orc)
    opq, gpq = orc.PQ(cents, T, 18, D), mse.ProductQuantizer(cents, T, 18, D)
    n, r, k = 300_000, 120, 10
    codes = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    scales = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)
    qs = (rng.standard_normal((9, D)) / np.sqrt(D)).astype(np.float32)
    luts = np.stack([opq.preprocess_query(q) for q in qs])
    gcodes = mse.Codes(codes, desc)
    approx = [opq.adc_desc(luts[j], codes, desc, scales) for j in range(9)]
    masks = {"all rows": np.ones(n, bool), "random 50 %": rng.random(n) < 0.5, "random 1/64": rng.random(n) < 1 / 64}

    def want(j, allowed, src=approx):
        ws, wi = orc.topk_from_scores(src[j][allowed], k)
        return ws, allowed[wi].astype(np.uint32)

    # the certificate of the 50 % filter, restated: eight-per-pass tables for queries 0 .. 7, four-per-pass tables for queries 0 .. 3
    half = np.flatnonzero(masks["random 50 %"])
    margins = []
    for per_pass in (8, 4):
        out, params = gpq.debug_group_max4_filtered(gcodes, masks["random 50 %"], luts[:per_pass], scales, per_pass=per_pass)
        for j in range(per_pass):
            assert params[j, 3] == 1
            margins.append(certificate_margin(out[j], params[j, 0], params[j, 1], params[j, 2], approx[j][half], half // 64, r, per_pass))
    print("certificate margins (score units):", [int(m) for m in margins])
    assert min(margins) > 0
    for name, mask in masks.items():
        allowed = np.flatnonzero(mask)
        f = mse.RowFilter(mask)
        for nq in (9, 8, 4):
            bs, bi = gpq.scan_topk_batch_filtered(gcodes, f, qs[:nq], r, k, None, scales, "scan")
            unc = gpq.last_uncertified
            print(name, nq, "uncertified:", unc)
            if name != "random 1/64":
                assert unc == 0, (name, nq)
            for j in range(nq):
                ws, wi = want(j, allowed)
                assert np.array_equal(bi[j], wi) and np.array_equal(bs[j], ws), (name, nq, j)
        f.close()
    tied = rng.integers(0, 256, size=(7, 64), dtype=np.uint8)[rng.integers(0, 7, size=n)]
    gt = mse.Codes(tied, None)
    tied_scores = [opq.asymmetric_dot_product(luts[j], tied) for j in range(8)]
    f = mse.RowFilter(masks["random 50 %"])
    for nq in (8, 4):
        bs, bi = gpq.scan_topk_batch_filtered(gt, f, qs[:nq], r, k, None, None, "scan")
        assert gpq.last_uncertified == nq
        for j in range(nq):
            ws, wi = want(j, half, tied_scores)
            assert np.array_equal(bi[j], wi) and np.array_equal(bs[j], ws), j
    f.close()
    # eight per pass is still in use: with the scan kernel's launches counted, an unfiltered batch of eight is ONE launch (4 + 4 would be two)
    gpq.scan_timing(2)
    gpq.scan_topk_batch(gcodes, qs[:8], r, k, None, scales)
    assert gpq.last_uncertified == 0 and gpq.scan_timing(0)[1] == 1


def test_live_index(gpu, mse, orc):
    """3 000 clustered rows with codes and descriptors behind a graph, half of them deleted: live_filter() is NOT deleted() (AND has_url
    on request); the filtered PQ scan and the filtered brute force under that filter equal the unfiltered calls on compact()'s outputs,
    ids sent through new_to_old; after insert_rows into freed slots a NEW filter includes them and the old one is unchanged."""
    n, r, k = 3000, 150, 10
    rng = np.random.default_rng(404)
    x = clustered_rows(orc, n, D, n_centres=20, seed=405)
    rows = orc.f16_bits(x)
    cents, T, dpc, _ = make_pq(orc, D, D // 64)
    opq, gpq = orc.PQ(cents, T, dpc, D), mse.ProductQuantizer(cents, T, dpc, D)
    codes = opq.quantize_batch(orc.f16_to_f32(rows))
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    scales = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)
    adj, deg = knn_graph(x, 16, rng)
    has_url = (rng.random(n) > 0.2).astype(np.uint8)
    entry = 1500
    has_url[entry] = 1
    vecs = mse.VectorList.from_f16s(rows, D)
    searcher = mse.Searcher(vecs)
    gcodes = mse.Codes(codes, desc)
    _, mcfg = cfgs(orc, mse, r=16, l=64, maxc=250)
    g = mse.DeviceGraph(mse.IndexGraph(adj, deg), has_url)
    qs = clustered_rows(orc, 6, D, n_centres=20, seed=406)
    qh = orc.f16_bits(qs)

    def rows_of(f):
        """the filter's allowed rows, read back through a search: brute force with k >= count returns every allowed row"""
        _, ids = searcher.bruteforce_topk(qh[:1], 1984, mse.MODE_EXACT, allow=f)
        return np.sort(ids[0][ids[0] != NONE])

    fresh = g.live_filter()
    assert len(fresh) == n and fresh.count == n                              # never deleted from: all ones
    dead = np.zeros(n, bool)
    dead[rng.choice(np.setdiff1d(np.arange(n), [entry]), n // 2, replace=False)] = True
    assert g.delete_rows(searcher, np.flatnonzero(dead), mcfg)["deleted"] == n // 2
    assert fresh.count == n                                                  # a snapshot
    live = g.live_filter()
    assert np.array_equal(g.deleted(), dead) and len(live) == n and live.count == n - n // 2
    assert np.array_equal(rows_of(live), np.flatnonzero(~dead))
    with_url = g.live_filter(and_has_url=True)
    assert np.array_equal(rows_of(with_url), np.flatnonzero(~dead & (has_url != 0))) and with_url.count == int((~dead & (has_url != 0)).sum())
    # the compacted index answers the same, through new_to_old
    cv, cc, cg, o2n, n2o = g.compact(searcher, gcodes)
    cs = mse.Searcher(cv)
    for s, s2 in ((None, None), (searcher, cs)):
        a_s, a_i = gpq.scan_topk_batch_filtered(gcodes, live, qs, r, k, s, scales)
        b_s, b_i = gpq.scan_topk_batch(cc, qs, r, k, s2, scales)
        assert (b_i != NONE).all() and np.array_equal(a_i, n2o[b_i]) and np.array_equal(a_s, b_s)
        for mode in MODES:
            m_s, m_i = gpq.scan_topk_batch_filtered(gcodes, live, qs, r, k, s, scales, mode)
            assert np.array_equal(m_s, a_s) and np.array_equal(m_i, a_i), mode
    lv = np.flatnonzero(~dead)
    bias = descriptor_bias(opq, codes, desc, scales)
    for j in range(6):                                                       # ... and both equal the oracle on the live rows
        ws, wi = oracle_topk(orc, opq, opq.preprocess_query(qs[j]), codes, bias, lv, r, k, rows, qh[j])
        assert np.array_equal(a_i[j], wi) and np.array_equal(a_s[j], ws), j
    for mode in (mse.MODE_EXACT, mse.MODE_MFMA):
        f_s, f_i = searcher.bruteforce_topk(qh, k, mode, allow=live)
        c_s, c_i = cs.bruteforce_topk(qh, k, mode)
        assert np.array_equal(f_i, n2o[c_i]) and np.array_equal(f_s, c_s), mode
    cg.close()
    # inserts into freed slots: a new filter has them, the old object keeps its rows
    slots = np.flatnonzero(dead)[:200].astype(np.uint32)
    new_rows = orc.f16_bits(clustered_rows(orc, 200, D, n_centres=20, seed=407))
    new_codes_desc = rng.integers(0, 256, size=(200, 4), dtype=np.uint8)
    assert g.insert_rows(searcher, slots, new_rows, mcfg, entry, gpq, gcodes, new_codes_desc)["inserted"] == 200
    after = g.live_filter()
    now_live = ~dead
    now_live[slots] = True
    assert after.count == int(now_live.sum()) and np.array_equal(rows_of(after), np.flatnonzero(now_live))
    assert live.count == n - n // 2 and np.array_equal(rows_of(live), np.flatnonzero(~dead))
    codes_now, desc_now = gcodes.read_rows(0, n, descriptors=True)
    rows_now = vecs.rows(0, n)
    assert np.array_equal(rows_now[slots], new_rows) and np.array_equal(desc_now[slots], new_codes_desc)
    bias_now = descriptor_bias(opq, codes_now, desc_now, scales)
    a_s, a_i = gpq.scan_topk_batch_filtered(gcodes, after, qs, r, k, searcher, scales)
    for j in range(6):
        ws, wi = oracle_topk(orc, opq, opq.preprocess_query(qs[j]), codes_now, bias_now, np.flatnonzero(now_live), r, k, rows_now, qh[j])
        assert np.array_equal(a_i[j], wi) and np.array_equal(a_s[j], ws), j
    for f in (fresh, live, with_url, after):
        f.close()
    g.close()


def test_errors_write_nothing(gpu, mse, orc):
    """A null filter, a filter longer than the codes, an unknown mode, r and k out of range: each an error whose message names the
    check, with the output buffers untouched."""
    from mse import ffi
    L = ffi.lib()
    rng = np.random.default_rng(5)
    cents, T, _, _ = make_pq(orc)
    gpq = mse.ProductQuantizer(cents, T, 18, D)
    n, k = 500, 10
    gcodes = mse.Codes(rng.integers(0, 256, size=(n, 64), dtype=np.uint8), None)
    ok, longer = mse.RowFilter(np.ones(n, bool)), mse.RowFilter(np.ones(n + 1, bool))
    q = (rng.standard_normal((2, D)) / np.sqrt(D)).astype(np.float32)
    cases = [(None, 100, k, 0, "null filter"), (longer._h, 100, k, 0, "longer than the codes"), (ok._h, 100, k, 7, "unknown mode"),
             (ok._h, 3000, k, 1, "r too large"), (ok._h, 100, 3000, 2, "r too large")]
    for fh, r, kk, mode, text in cases:
        scores = np.full(2 * 3000, 0x5A5A5A5A5A5A5A5A, np.int64)
        ids = np.full(2 * 3000, 0x5A5A5A5A, np.uint32)
        sp, ip = scores.ctypes.data_as(ffi.i64p), ids.ctypes.data_as(ffi.u32p)
        qp = q.ctypes.data_as(ffi.f32p)
        assert L.mse_pq_scan_topk_batch_filtered(gpq._h, gcodes._h, fh, None, qp, 2, None, r, kk, mode, sp, ip) != 0
        assert text in ffi.last_error(), (text, ffi.last_error())
        assert L.mse_pq_scan_topk_filtered(gpq._h, gcodes._h, fh, None, qp, None, r, kk, mode, sp, ip) != 0
        assert text in ffi.last_error(), (text, ffi.last_error())
        assert L.mse_pq_scan_topk_block_filtered(gpq._h, gcodes._h, fh, None, qp, 2, None, r, kk, mode, 0, C.c_void_p(scores.ctypes.data)) != 0
        assert text in ffi.last_error(), (text, ffi.last_error())
        assert (scores == 0x5A5A5A5A5A5A5A5A).all() and (ids == 0x5A5A5A5A).all(), text
    out = np.full(8, 0x5A5A5A5A5A5A5A5A, np.int64)
    lut = np.zeros(64 * 256, np.float32)
    for fh, text in ((None, "null filter"), (longer._h, "longer than the codes")):
        assert L.mse_debug_pq_group_max_filtered(gpq._h, gcodes._h, fh, lut.ctypes.data_as(ffi.f32p), None, None, out.ctypes.data_as(ffi.i64p), None) != 0
        assert text in ffi.last_error() and (out == 0x5A5A5A5A5A5A5A5A).all()
    with pytest.raises(KeyError):
        gpq.scan_topk_filtered(gcodes, ok, q[0], 100, k, mode="fastest")
    ok.close()
    longer.close()


def test_auto_equals_the_plan_on_both_sides(gpu, mse, orc):
    """mode="auto" is the explicit call at filtered_plan's answer.  The two filters sit on either side of the crossover as the plan
    function itself places it (found by bisection over its answers, not from a constant)."""
    rng = np.random.default_rng(17)
    cents, T, _, _ = make_pq(orc)
    opq, gpq = orc.PQ(cents, T, 18, D), mse.ProductQuantizer(cents, T, 18, D)
    n, r, k = 2_000_000, 64, 10                                              # (large enough for the plan to have a LIST side at all)
    codes = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    gcodes = mse.Codes(codes, None)
    for nq in (1, 5):
        qs = (rng.standard_normal((nq, D)) / np.sqrt(D)).astype(np.float32)
        assert gpq.filtered_plan(n, 0, nq) == "list" and gpq.filtered_plan(n, n, nq) == "scan"
        lo, hi = 0, n                                                       # plan(lo) == "list", plan(hi) == "scan"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if gpq.filtered_plan(n, mid, nq) == "list" else (lo, mid)
        for count, side in ((lo, "list"), (hi, "scan")):
            assert gpq.filtered_plan(n, count, nq) == side
            mask = np.zeros(n, bool)
            mask[rng.choice(n, count, replace=False)] = True
            f = mse.RowFilter(mask)
            auto = gpq.scan_topk_batch_filtered(gcodes, f, qs, r, k)
            explicit = gpq.scan_topk_batch_filtered(gcodes, f, qs, r, k, mode=side)
            assert np.array_equal(auto[0], explicit[0]) and np.array_equal(auto[1], explicit[1])
            allowed = np.flatnonzero(mask)
            for j in range(nq):
                ws, wi = oracle_topk(orc, opq, opq.preprocess_query(qs[j]), codes, None, allowed, r, k)
                assert np.array_equal(auto[1][j], wi) and np.array_equal(auto[0][j], ws)
            f.close()
