"""Oracle parity of the device-resident beam search (beam_search_kernel) across the whole range the host accepts: beamwidth 1..8,
search_list 1..1024, max_deg up to 128 (merged indexes: every record spills into two shards), ADC scoring with and without the
descriptor bias and exact scoring, the one-, four-, eight- and sixteen-wave forms, bit maps and hash tables as visited sets.

An iteration lays out beam x max_deg adjacency slots; the cases straddle 512 of them (what the ADC kernel's register staging holds)
up to the largest, 8 x 128 = 1024.  Every case compares, query by query, the search list (ids and scores), the visited records in
fetch order (ids and exact scores), `cmps` and `pq_cmps` with the oracle's restatement of query_disk_index::greedy_search."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pq_index_graph import D, clustered_rows, knn_graph, train_pq

pytestmark = pytest.mark.gpu

N = 4000                                   # rows: enough for a list of 1024 to fill
SCALES = np.array([0.5, 0, -0.25, 1.0], np.float32) / np.float32(512)
ID_NONE = 0xFFFFFFFF


class Index:
    """One clustered base, its codec, codes and descriptors, and graphs of several widths over it (built on first use).  Search
    results and oracle answers are kept per case, so that the wave-form test re-checks the cases the parametrized tests ran."""

    def __init__(self, orc, mse):
        self.orc, self.mse = orc, mse
        rng = np.random.default_rng(41)
        self.x = clustered_rows(orc, N, n_centres=24, seed=41)
        self.base = orc.f16_bits(self.x)
        self.cents, self.T = cents, T = train_pq(orc, self.x[:1500], iters=1)
        self.opq, self.gpq = orc.PQ(cents, T, 18, D), mse.ProductQuantizer(cents, T, 18, D)
        # codes quantized on the device (test_codec_matches_oracle holds that codec to the oracle's): inputs of both sides here
        self.codes = self.gpq.quantize_batch(orc.f16_to_f32(self.base))
        self.desc = rng.integers(0, 256, size=(N, 4), dtype=np.uint8)
        self.searcher = mse.Searcher(mse.VectorList.from_f16s(self.base, D))
        self.gcodes = mse.Codes(self.codes, self.desc)
        s = self.x @ self.x.T
        np.fill_diagonal(s, -np.inf)
        self.near = np.argsort(-s, axis=1)[:, :128].astype(np.uint32)
        self._graphs, self._queries, self._luts, self._got, self._want = {}, {}, {}, {}, {}

    def graph(self, md):
        """Nearest neighbours + random edges, ragged: about 5 % of the nodes have no neighbours, a fifth have max_deg of them.
        Ids repeat inside lists (and across the nodes of a beam: neighbours share neighbours); slots past a node's degree hold
        ids >= n, which the search must ignore."""
        if md not in self._graphs:
            rng = np.random.default_rng(1000 + md)
            long_edges = max(2, md // 10)
            adj = np.concatenate([self.near[:, :md - long_edges], rng.integers(0, N, size=(N, long_edges))], axis=1).astype(np.uint32)
            degs = rng.integers(md // 2, md + 1, size=N).astype(np.uint32)
            degs[rng.choice(N, N // 5, replace=False)] = md
            degs[rng.choice(N, N // 20, replace=False)] = 0
            rep = rng.choice(N, N // 10, replace=False)                      # an id listed twice in one list
            for i in rep:
                if degs[i] >= 2:
                    a, b = sorted(rng.choice(int(degs[i]), 2, replace=False))
                    adj[i, b] = adj[i, a]
            pad = np.arange(md)[None, :] >= degs[:, None]
            adj[pad] = np.where(rng.random(int(pad.sum())) < 0.5, ID_NONE, N + rng.integers(0, 1 << 20, int(pad.sum()))).astype(np.uint32)
            self._graphs[md] = (adj, degs, self.mse.DeviceGraph(self.mse.IndexGraph(adj, degs)))
        return self._graphs[md]

    def queries(self, nq, seed):
        if (nq, seed) not in self._queries:
            rng = np.random.default_rng(seed)
            qs = clustered_rows(self.orc, nq, n_centres=24, seed=seed)
            self._queries[(nq, seed)] = (qs, rng.integers(0, N, size=nq).astype(np.uint32))
        return self._queries[(nq, seed)]

    def luts(self, nq, seed):
        """the queries' distance tables (the oracle's)"""
        if (nq, seed) not in self._luts:
            self._luts[(nq, seed)] = np.stack([self.opq.preprocess_query(q) for q in self.queries(nq, seed)[0]])
        return self._luts[(nq, seed)]

    def inputs(self, case):
        beam, md, adc, bias, L, nq, seed = case
        adj, degs, dg = self.graph(md)
        qs, starts = self.queries(nq, seed)
        qh = self.orc.f16_bits(qs)
        luts = self.luts(nq, seed) if adc else np.zeros((nq, 64 * 256), np.float32)   # (not read by exactly scored searches)
        live = np.flatnonzero(degs > 0)
        starts = live[starts % len(live)].astype(np.uint32)
        starts[0] = np.flatnonzero(degs == 0)[0]                           # a start without neighbours: the search ends at once
        if nq > 1:
            starts[1] = np.flatnonzero(degs == md)[seed % 7]                # a start with a full list
        return adj, degs, dg, qh, luts, starts, (SCALES if bias else None), not adc

    def search(self, case, **kw):
        """disk_search_batch of a case as padded arrays (as_arrays=True)"""
        beam, md, adc, bias, L, nq, seed = case
        adj, degs, dg, qh, luts, starts, scales, disable_pq = self.inputs(case)
        return self.mse.disk_search_batch(self.searcher, self.gpq, self.gcodes, dg, starts, qh, luts, scales, disable_pq, beam,
                                          search_list=L, visited_cap=kw.get("visited_cap", N), as_arrays=True)

    def got(self, case):
        if case not in self._got:
            self._got[case] = self.search(case)
        return self._got[case]

    def want(self, case, i):
        """the oracle's (buffer ids, buffer scores, visited ids, visited scores, cmps, pq_cmps) for query i of a case"""
        if (case, i) not in self._want:
            beam, md, adc, bias, L, nq, seed = case
            adj, degs, dg, qh, luts, starts, scales, disable_pq = self.inputs(case)
            obuf, ovids, ovsc, ocm, opc = self.orc.disk_greedy_search(self.base, adj, degs, self.codes, self.desc, int(starts[i]), qh[i],
                                                                      luts[i], scales, disable_pq, beam, L, None)
            self._want[(case, i)] = (obuf.ids.copy(), obuf.scores.copy(), ovids, ovsc, ocm, opc)
        return self._want[(case, i)]


@pytest.fixture(scope="module")
def ix(gpu, orc, mse):
    return Index(orc, mse)


def row(res, i):
    """query i of a padded result: the valid parts only"""
    n, nv = int(res["buf_len"][i]), int(res["n_visited"][i])
    return (res["buf_ids"][i, :n], res["buf_scores"][i, :n], res["visited_ids"][i, :nv], res["visited_scores"][i, :nv],
            int(res["cmps"][i]), int(res["pq_cmps"][i]))


def assert_row(got, want, i):
    bi, bs, vi, vs, cm, pc = got
    wi, ws, wvi, wvs, wcm, wpc = want
    assert (cm, pc) == (wcm, wpc), i
    assert np.array_equal(bi, wi) and np.array_equal(bs, ws), i
    assert np.array_equal(vi, wvi) and np.array_equal(vs, wvs), i


def check_case(ix, case, res=None, stride=1):
    res = ix.got(case) if res is None else res
    nq = res["buf_len"].shape[0]
    for i in sorted(set(range(0, nq, stride)) | {nq - 1}):
        assert_row(row(res, i), ix.want(case, i), i)
    return res


# (beam, max_deg, adc, bias, search_list, queries, seed): beam x max_deg straddles the 512 slots the ADC kernel stages in registers
CASES = [
    (8, 64, True, True, 65, 6, 1),         # 512 exactly
    (7, 73, True, False, 63, 6, 2),        # 511, max_deg not a multiple of 64
    (7, 74, True, True, 64, 6, 3),         # 518
    (5, 128, True, False, 257, 5, 4),      # 640
    (6, 100, True, True, 256, 5, 5),       # 600
    (8, 100, True, False, 2, 6, 6),        # 800
    (8, 128, True, True, 1024, 4, 7),      # 1024, the widest iteration and the longest list
    (8, 128, True, False, 1, 6, 8),        # a list of one
    (1, 128, True, True, 100, 6, 9),       # L = 100: flags ending at 4 mod 8 before the LDS regions were aligned
    (8, 128, False, True, 300, 4, 10),     # exact scoring at full width
    (6, 100, False, False, 1024, 3, 11),
]
WIDEST = CASES[6]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_deg%d_%s%s_L%d" % (c[0], c[1], "adc" if c[2] else "exact", "_bias" if c[3] else "", c[4]))
def test_beam_search_envelope_matches_oracle(ix, case):
    """Four-wave kernel (every ADC-scored search, and exactly scored batches of up to 1024 queries), ragged graphs with empty and
    full lists, repeated ids and padding ids >= n past the degrees: every query equals the oracle."""
    beam, md, adc, bias, L, nq, seed = case
    res = check_case(ix, case)
    assert res["buf_len"][0] == 1 and res["n_visited"][0] <= 1        # the start without neighbours
    if L == 1024:
        assert np.all(res["buf_len"][1:] == L)                          # the longest list really filled
    if adc:
        assert np.all(res["pq_cmps"][1:] > 0)                           # every other search scored neighbours through the table
    else:
        assert np.all(res["pq_cmps"] == 0)


def test_one_wave_form_at_its_limits(ix):
    """More than 1024 exactly scored queries with search_list and pre-buffer <= 256 run one wave per query: nq = 1025, L = 256,
    beam 2 x degree 128 (a pre-buffer of 256).  A fixed stride of the queries is checked, the last one included."""
    case = (2, 128, False, True, 256, 1025, 12)
    res = check_case(ix, case, stride=32)
    assert np.all(res["buf_len"][1:] == 256)


@pytest.mark.parametrize("bits", [None, "12"])
def test_hash_visited_sets_at_full_width(ix, monkeypatch, bits):
    """Visited sets as open-addressing tables (MSE_VISITED_MODE=hash) at the widest ADC case: the oracle's answers; with a
    4096-slot table the searches outgrow it (more than 2048 ids in visited_adjacent) and the call repeats with bit maps."""
    monkeypatch.setenv("MSE_VISITED_MODE", "hash")
    if bits:
        monkeypatch.setenv("MSE_VISITED_TABLE_BITS", bits)
    check_case(ix, WIDEST, res=ix.search(WIDEST))
    adj, degs, dg, qh, luts, starts, scales, disable_pq = ix.inputs(WIDEST)
    vi = ix.want(WIDEST, 1)[2]                                            # every fetched node (no record lacks a URL here)
    adjacent = set(np.concatenate([adj[v, :degs[v]] for v in vi]).tolist()) | {int(starts[1])}
    assert len(adjacent) > 2048


def test_truncated_visited_records(ix):
    """visited_cap below a search's n_visited: the first visited_cap records are the oracle's first ones, n_visited counts them all,
    and the search itself is not cut short."""
    cap = 37
    res = ix.search(WIDEST, visited_cap=cap)
    for i in range(res["buf_len"].shape[0]):
        bi, bs, vi, vs, cm, pc = ix.want(WIDEST, i)
        assert int(res["n_visited"][i]) == len(vi), i
        m = min(cap, len(vi))
        assert np.array_equal(res["visited_ids"][i, :m], vi[:m]) and np.array_equal(res["visited_scores"][i, :m], vs[:m]), i
        n = int(res["buf_len"][i])
        assert np.array_equal(res["buf_ids"][i, :n], bi) and np.array_equal(res["buf_scores"][i, :n], bs), i
        assert (int(res["cmps"][i]), int(res["pq_cmps"][i])) == (cm, pc), i
    assert int(res["n_visited"].max()) > cap


def test_request_path_at_full_width(ix, mse):
    """disk_query_topk at ADC beam 8, degree 128, L 1024 and a large k: the visited records ordered by exact score (id ascending on
    equal scores), cut to k and padded, and the counters, against the oracle's search."""
    case, k = WIDEST, 1500
    adj, degs, dg, qh, luts, starts, scales, disable_pq = ix.inputs(case)
    ids, scores, stats = mse.disk_query_topk(ix.searcher, ix.gpq, ix.gcodes, dg, qh, k, starts, luts, scales, disable_pq, case[0], case[4])
    for i in range(len(qh)):
        _, _, ovids, ovsc, ocm, opc = ix.want(case, i)
        order = np.array(sorted(range(len(ovids)), key=lambda j: (-int(ovsc[j]), int(ovids[j]))), np.int64)
        want_ids = np.full(k, ID_NONE, np.uint32)
        want_sc = np.full(k, np.iinfo(np.int64).min, np.int64)
        m = min(k, len(order))
        want_ids[:m] = ovids[order[:m]]
        want_sc[:m] = ovsc[order[:m]]
        assert np.array_equal(ids[i], want_ids) and np.array_equal(scores[i], want_sc), i
        assert (int(stats["cmps"][i]), int(stats["pq_cmps"][i]), int(stats["n_visited"][i])) == (ocm, opc, len(ovids)), i


def test_ties_at_full_width(orc, mse):
    """The tie-heavy base of test_beam_search_among_many_equal_scores_matches_oracle (a third of the rows are exact copies: equal
    exact AND equal ADC scores; a fifth of the queries are rows) at ADC beam 8 x degree 128: iterations of up to 1024 offers go down
    the sequential replay path.  Equal scores really sit inside the lists."""
    rng = np.random.default_rng(78)
    n, deg = 2400, 128
    x = clustered_rows(orc, n, n_centres=12)
    src = rng.integers(0, n, size=n // 3)
    dst = rng.choice(n, size=n // 3, replace=False)
    x[dst] = x[src]
    base = orc.f16_bits(x)
    cents, T = train_pq(orc, x[:1500], iters=1)
    opq, gpq = orc.PQ(cents, T, 18, D), mse.ProductQuantizer(cents, T, 18, D)
    codes = gpq.quantize_batch(orc.f16_to_f32(base))
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    desc[dst] = desc[src]
    adj, degs = knn_graph(x, deg, rng, long_edges=12)
    adj[7, 100] = adj[7, 2]
    searcher = mse.Searcher(mse.VectorList.from_f16s(base, D))
    gcodes = mse.Codes(codes, desc)
    dgraph = mse.DeviceGraph(mse.IndexGraph(adj, degs))
    replayed = 0
    for L, nq in ((40, 16), (300, 6)):
        qs = clustered_rows(orc, nq, n_centres=12, seed=310 + L)
        qs[::4] = x[rng.integers(0, n, size=len(qs[::4]))]
        qh = orc.f16_bits(qs)
        luts = np.stack([opq.preprocess_query(q) for q in qs])
        starts = rng.integers(0, n, size=nq).astype(np.uint32)
        got = mse.disk_search_batch(searcher, gpq, gcodes, dgraph, starts, qh, luts, SCALES, False, 8, search_list=L, visited_cap=n)
        for i in range(nq):
            obuf, ovids, ovsc, ocm, opc = orc.disk_greedy_search(base, adj, degs, codes, desc, int(starts[i]), qh[i], luts[i], SCALES,
                                                                  False, 8, L, None)
            bi, bs, vi, vs, cm, pc = got[i]
            assert (cm, pc) == (ocm, opc), (L, i)
            assert np.array_equal(bi, obuf.ids) and np.array_equal(bs, obuf.scores), (L, i)
            assert np.array_equal(vi, ovids) and np.array_equal(vs, ovsc), (L, i)
            replayed += int(len(np.unique(bs)) < len(bs))
    assert replayed > 0


def test_parameter_limits(ix, mse):
    """beamwidth 1..8, search_list 1..1024 and max_deg <= 128 are the limits; outside them the call fails instead of searching."""
    case = (2, 64, True, True, 32, 2, 13)
    adj, degs, dg, qh, luts, starts, scales, _ = ix.inputs(case)
    args = (ix.searcher, ix.gpq, ix.gcodes)
    for beam, L in ((0, 32), (9, 32), (2, 0), (2, 1025)):
        with pytest.raises(mse.MseError):
            mse.disk_search_batch(*args, dg, starts, qh, luts, scales, False, beam, search_list=L, visited_cap=N)
        with pytest.raises(mse.MseError):
            mse.disk_query_topk(*args, dg, qh, 10, starts, luts, scales, False, beam, L)
    wide = np.full((N, 129), ID_NONE, np.uint32)                         # 129 columns, the same lists
    wide[:, :adj.shape[1]] = adj
    g129 = mse.DeviceGraph(mse.IndexGraph(wide, degs))
    with pytest.raises(mse.MseError):
        mse.disk_search_batch(*args, g129, starts, qh, luts, scales, False, 2, search_list=32, visited_cap=N)
    with pytest.raises(mse.MseError):
        mse.disk_query_topk(*args, g129, qh, 10, starts, luts, scales, False, 2, 32)
    # the same call inside the limits goes through
    mse.disk_search_batch(*args, dg, starts, qh, luts, scales, False, 8, search_list=1024, visited_cap=N)


# A child process runs the cases with MSE_BEAM_WAVES forcing a form (the library reads it once per process) and saves its arrays.
_CHILD = r"""
import sys
import numpy as np
try:
    import torch  # noqa: F401  -- before libmse_hip.so (tests/conftest.py)
except Exception:
    pass
sys.path.insert(0, sys.argv[1])
import mse
z = np.load(sys.argv[2])
d = int(z["d"])
searcher = mse.Searcher(mse.VectorList.from_f16s(z["base"], d))
gpq = mse.ProductQuantizer(z["cents"], z["T"], 18, d)
gcodes = mse.Codes(z["codes"], z["desc"])
out = {}
for c in range(int(z["n_cases"])):
    p = lambda k: z["c%d_%s" % (c, k)]
    beam, L, disable_pq, bias = (int(v) for v in p("params"))
    dg = mse.DeviceGraph(mse.IndexGraph(p("adj"), p("degs")))
    res = mse.disk_search_batch(searcher, gpq, gcodes, dg, p("starts"), p("qh"), p("luts"), z["scales"] if bias else None, bool(disable_pq),
                                beam, search_list=L, visited_cap=len(z["base"]), as_arrays=True)
    for k, v in res.items():
        out["c%d_%s" % (c, k)] = v
np.savez(sys.argv[3], **out)
"""
WAVE_CASES = [WIDEST, CASES[2], CASES[4], CASES[7], CASES[9]]


def test_eight_and_sixteen_wave_forms(ix, tmp_path):
    """MSE_BEAM_WAVES=8 / 16 (answer-preserving, search_launch): a fresh process per form, one after the other; each returns, for
    every query, what the four-wave form returns -- which equals the oracle."""
    data = {"d": D, "base": ix.base, "codes": ix.codes, "desc": ix.desc, "scales": SCALES, "n_cases": len(WAVE_CASES), "cents": ix.cents,
            "T": ix.T}
    for c, case in enumerate(WAVE_CASES):
        adj, degs, dg, qh, luts, starts, scales, disable_pq = ix.inputs(case)
        data.update({"c%d_adj" % c: adj, "c%d_degs" % c: degs, "c%d_qh" % c: qh, "c%d_luts" % c: luts, "c%d_starts" % c: starts,
                     "c%d_params" % c: np.array([case[0], case[4], int(disable_pq), int(case[3])])})
        check_case(ix, case)                                              # the four-wave answers equal the oracle
    inp = str(tmp_path / "in.npz")
    np.savez(inp, **data)
    for waves in (8, 16):
        env = dict(os.environ, MSE_BEAM_WAVES=str(waves))
        out = str(tmp_path / ("out%d.npz" % waves))
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _CHILD, os.path.join(ROOT, "meme-search-engine_amd"), inp, out]
        r = subprocess.run(cmd, env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, (waves, r.returncode, r.stderr[-3000:])
        z = np.load(out)
        for c, case in enumerate(WAVE_CASES):
            res = {k: z["c%d_%s" % (c, k)] for k in ("buf_ids", "buf_scores", "buf_len", "visited_ids", "visited_scores", "n_visited", "cmps", "pq_cmps")}
            four = ix.got(case)
            for i in range(res["buf_len"].shape[0]):
                assert_row(row(res, i), row(four, i), (waves, case, i))
