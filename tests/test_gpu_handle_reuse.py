"""Long-lived handles: a call's answer and statistics depend on its arguments and the handle's rows only, never on the calls before it.

A server keeps one Searcher, one ScalarQuantizerIndex (and one ProductQuantizer: tests/test_gpu_pq_handle_reuse.py) for its lifetime, and
each of them lives on scratch that is reused between calls and neither preserved nor cleared (runtime.h DevBuf::ensure).  A kernel that
reads one column, group, candidate slot or padding row more than the current call wrote reads, on a fresh handle, whatever hipMalloc
returned -- and on a long-lived one the previous call's values.  So every test here drives ONE handle through a sequence that alternates

  POISON calls: many queries, a large k, every row scoring high -- the scratch is left full of values and valid ids that would win, and
  PROBE calls:  few or differently shaped, every true score below every poison score,

and compares every call bit for bit (i64 scores, ids, padding) with the CPU oracle and with the same single call on a fresh handle,
statistics included.  That the poison is effective is asserted on the oracle's numbers before the first GPU call: the smallest poison
score is above the largest probe score.  Expectations are cut from one oracle score matrix per query pool (orc.score_all ->
orc.topk_from_scores, over the allowed rows for filtered steps).

Brute force: 9041 x 1152 rows -- 35 tiles of 256 rows and 81 more, so every tail is ragged, and the size at which
set_sparse_maxima("forced", 3) still takes the sparse form (48 sample groups, enough for k = 10 and too few for k = 100, which goes dense
by itself).  At this size the tournament needs no upper level (16384 keys are selected from directly), so `levels` is not reached here;
tests/test_gpu_topk_select.py holds that part.  A coalesced MODE_AUTO call runs on the base's worker searcher and leaves the caller's
statistics alone, so those steps are compared by answer only, against a fresh base."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
D = 1152
N = 9041
I64_MIN = np.iinfo(np.int64).min
ID_NONE = 0xFFFFFFFF
SPARSE = ("forced", 3)


class Brute:
    """The base, its query pools, the oracle's score matrix of every pool, and the filters."""

    def __init__(self, orc, mse):
        self.orc, self.mse = orc, mse
        rng = np.random.default_rng(20261)
        u = np.ones(D) / np.sqrt(D)
        rows = rng.standard_normal((N, D)) / np.sqrt(D) + 0.5 * u
        self.base = orc.f16_bits(rows.astype(np.float32))
        # 40 exact copies of one row, one per 200 rows: 40 distinct 32-row AND 64-row groups.  A query equal to that row finds more
        # tied groups than the first round takes (18), so its first certificate fails and the search widens.
        self.copies = np.arange(40) * 200 + 7
        self.base[self.copies] = self.base[self.copies[0]]
        noise = lambda m: rng.standard_normal((m, D)) / np.sqrt(D)
        tie = np.tile(self.base[self.copies[0]], (12, 1))
        self.pools = {"poison": orc.f16_bits((4 * u + noise(330)).astype(np.float32)),
                      "probe": orc.f16_bits((-4 * u + noise(320)).astype(np.float32)),
                      "tie": tie}
        self.scores = {name: np.stack([orc.score_all(self.base, q) for q in pool]) for name, pool in self.pools.items()}
        for a in list(self.pools.values()) + list(self.scores.values()) + [self.base]:
            a.setflags(write=False)
        self.masks = {"dense": rng.random(N) < 0.8, "seventeen": np.zeros(N, bool), "empty": np.zeros(N, bool)}
        self.masks["seventeen"][rng.choice(N, 17, replace=False)] = True
        self._want = {}
        self.vl = self.filters = None
        self._checked = False

    def check_poison(self):
        """every row's score under every poison (and tie) query is above every row's score under every probe query"""
        if self._checked:
            return
        lo = min(int(self.scores["poison"].min()), int(self.scores["tie"].min()))
        hi = int(self.scores["probe"].max())
        print("smallest poison score %.3f, largest probe score %.3f (units of 2^32)" % (lo / 2.0 ** 32, hi / 2.0 ** 32))
        assert lo > 0 > hi
        self._checked = True

    def device(self):
        if self.vl is None:
            self.vl = self.mse.VectorList.from_f16s(self.base, D)
            self.filters = {name: self.mse.RowFilter(m) for name, m in self.masks.items()}
        return self.vl

    def queries(self, parts):
        return np.ascontiguousarray(np.concatenate([self.pools[p][lo:hi] for p, lo, hi in parts]))

    def want(self, parts, k, allow=None):
        """the oracle's ([nq, k] scores, [nq, k] ids), slots past the (allowed) rows (INT64_MIN, ID_NONE)"""
        key = (tuple(parts), k, allow)
        if key not in self._want:
            rows = np.concatenate([self.scores[p][lo:hi] for p, lo, hi in parts])
            allowed = None if allow is None else np.flatnonzero(self.masks[allow])
            ws = np.full((len(rows), k), I64_MIN, np.int64)
            wi = np.full((len(rows), k), ID_NONE, np.uint32)
            for j, sc in enumerate(rows):
                if allowed is None:
                    s, i = self.orc.topk_from_scores(sc, min(k, N))
                elif len(allowed):
                    s, i = self.orc.topk_from_scores(sc[allowed], min(k, len(allowed)))
                    i = allowed[i].astype(np.uint32)
                else:
                    continue
                ws[j, :len(s)], wi[j, :len(i)] = s, i
            self._want[key] = (ws, wi)
        return self._want[key]


@pytest.fixture(scope="module")
def bf(orc, mse):
    return Brute(orc, mse)


def step(parts, k, mode="mfma", sparse=None, allow=None, widened=None, sparse_passes=None):
    """One brute-force call: parts = ((pool, first, last), ...), the queries side by side.  widened / sparse_passes: what the call's
    statistics must say (None: only that they equal the fresh handle's)."""
    if isinstance(parts[0], str):
        parts = (parts,)
    return dict(parts=tuple(parts), k=k, mode=mode, sparse=sparse, allow=allow, widened=widened, sparse_passes=sparse_passes)


def call(bf, s, st):
    mse = bf.mse
    s.set_sparse_maxima(*(st["sparse"] or ("auto", 3)))
    mode = {"mfma": mse.MODE_MFMA, "exact": mse.MODE_EXACT}[st["mode"]]
    allow = bf.filters[st["allow"]] if st["allow"] else None
    sc, ids = s.bruteforce_topk(bf.queries(st["parts"]), st["k"], mode, allow=allow)
    return sc, ids, s.last_stats()


def run_sequence(bf, seq, searcher=None):
    """every step on the long-lived searcher == the oracle == the same single call on a fresh searcher (answers and statistics)"""
    bf.check_poison()
    vl = bf.device()
    s = searcher or bf.mse.Searcher(vl)
    for n, st in enumerate(seq):
        ws, wi = bf.want(st["parts"], st["k"], st["allow"])
        sc, ids, stats = call(bf, s, st)
        where = (n, st["parts"], st["k"], st["mode"], st["sparse"], st["allow"])
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), ("long-lived handle differs from the oracle", where, stats)
        fresh = bf.mse.Searcher(vl)
        fsc, fids, fstats = call(bf, fresh, st)
        fresh.close()
        assert np.array_equal(fids, wi) and np.array_equal(fsc, ws), ("fresh handle differs from the oracle", where)
        assert stats == fstats, (where, stats, fstats)
        if st["widened"] is not None:
            assert (stats["widened_queries"] > 0) == st["widened"], (where, stats)
        if st["sparse_passes"] is not None:
            assert stats["sparse_passes"] == st["sparse_passes"] and stats["sparse_fallbacks"] == 0, (where, stats)
    if searcher is None:
        s.close()


P, Q, T = "poison", "probe", "tie"
MAIN = [
    # lists, counts and thresholds of the previous 320-query pass
    step((P, 0, 320), 100, sparse=SPARSE, sparse_passes=0),             # 48 sample groups < k: dense by itself, 64-row groups
    step((P, 0, 320), 10, sparse=SPARSE, sparse_passes=1),
    step((Q, 0, 320), 10, sparse=SPARSE, sparse_passes=1),
    # 64-row groups of a 320-query pass -> pad 128 and 32-row groups: another layout of the group maxima
    step((P, 0, 320), 10),
    step((Q, 0, 3), 10),
    # 320 + 10 in one call, columns side by side -> pad 192 -> 256 -> 128
    step((P, 0, 330), 10),
    step((Q, 0, 130), 10),
    step((Q, 0, 256), 10),
    step((Q, 0, 9), 10),
    # k = 1000 <-> k = 1: selections full of valid ids
    step((P, 0, 40), 1000),
    step((Q, 0, 40), 1),
    step((P, 40, 80), 1),
    step((Q, 40, 80), 1000),
    # ties that widen -> fewer clean queries: wq / wg / widx / wout
    step((T, 0, 12), 10, widened=True),
    step((Q, 0, 5), 10, widened=False),
    step(((P, 0, 308), (T, 0, 12)), 10, sparse=SPARSE, sparse_passes=1, widened=True),   # ... and the compact lists of the sparse form
    step((Q, 0, 300), 10, sparse=SPARSE, sparse_passes=1),
    # unfiltered poison -> three filters (stale ids must not come back as padding) -> unfiltered probe
    step((P, 0, 40), 100),
    step((Q, 0, 40), 32, allow="dense"),
    step((Q, 0, 9), 32, mode="exact", allow="seventeen"),                # the id-list pass: 17 results, then (INT64_MIN, ID_NONE)
    step((Q, 0, 40), 32, allow="seventeen"),                             # the masked scan over the same 17 rows
    step((Q, 0, 5), 32, allow="empty"),
    step((Q, 0, 7), 10),
]


def test_poison_then_probe(gpu, bf):
    run_sequence(bf, MAIN)


def test_poison_then_probe_in_reverse(gpu, bf):
    """the same calls last to first: small before large, so buffers grow in the middle of the sequence"""
    run_sequence(bf, MAIN[::-1])


def test_filtered_padding_is_padding(gpu, bf):
    """what the sequences rely on, spelled out: 17 allowed rows and k = 32 give 17 results and 15 x (INT64_MIN, ID_NONE)"""
    ws, wi = bf.want(((Q, 0, 9),), 32, "seventeen")
    assert np.all(wi[:, 17:] == ID_NONE) and np.all(ws[:, 17:] == I64_MIN) and np.all(bf.masks["seventeen"][wi[:, :17]])
    assert 0.75 * N < bf.masks["dense"].sum() < 0.85 * N


def test_exact_mode_scores_ranks_and_score_rows_share_scratch(gpu, bf, orc, mse):
    """MODE_EXACT, scores(), ranks() and score_rows() all go through s->scores and q_stage: 8 poison queries at k = 1000, then one
    probe at k = 3, with the row calls between them -- an id past the base among them."""
    bf.check_poison()
    s = mse.Searcher(bf.device())
    ids = np.array([5, N - 1, 0, 4242, 7, 207], np.uint32)
    outside = np.array([3, N, N - 1, ID_NONE, 12], np.uint32)

    def row_calls(pool, j):
        q, sc = bf.pools[pool][j], bf.scores[pool][j]
        assert np.array_equal(s.scores(q), sc), (pool, j)
        assert np.array_equal(s.ranks(q, ids), orc.ranks_from_scores(sc)[ids]), (pool, j)
        got = s.score_rows(outside, q)
        assert np.array_equal(got[[0, 2, 4]], sc[[3, N - 1, 12]]) and np.all(got[[1, 3]] == I64_MIN), (pool, j)

    run_sequence(bf, [step((P, 0, 8), 1000, mode="exact")], searcher=s)
    row_calls(Q, 0)
    run_sequence(bf, [step((Q, 0, 1), 3, mode="exact")], searcher=s)
    row_calls(P, 3)
    row_calls(Q, 1)
    run_sequence(bf, [step((Q, 1, 2), 3, mode="exact"), step((P, 0, 40), 1000), step((Q, 2, 3), 3, mode="exact"),
                      step((Q, 0, 8), 1, mode="exact"), step((P, 8, 16), 1000, mode="exact")], searcher=s)
    row_calls(Q, 2)
    s.close()


def test_auto_mode_through_the_bases_dispatcher(gpu, bf, mse):
    """MODE_AUTO with up to 320 host queries goes to the base's coalescer, whose worker searcher lives as long as the base: 40 poison
    queries, then 2 probes (its exact pass), 40 probes, 1 probe -- against the oracle and against a base of its own per call."""
    bf.check_poison()
    vl = bf.device()
    s = mse.Searcher(vl)
    for parts, k in (((P, 0, 40), 100), ((Q, 0, 2), 10), ((P, 0, 320), 10), ((Q, 0, 40), 10), ((Q, 5, 6), 1)):
        ws, wi = bf.want((parts,), k)
        sc, ids = s.bruteforce_topk(bf.queries((parts,)), k)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), (parts, k)
        fvl = mse.VectorList.from_f16s(bf.base, D)
        fs = mse.Searcher(fvl)
        fsc, fids = fs.bruteforce_topk(bf.queries((parts,)), k)
        fs.close()
        fvl.close()
        assert np.array_equal(fids, wi) and np.array_equal(fsc, ws), ("fresh base", parts, k)
    s.close()


def test_device_queries_off_a_16_byte_boundary(gpu, bf, mse):
    """bruteforce_topk_dev with queries at an address that is a multiple of 2 and not of 16: the rows are copied once through q_stage.
    40 poison queries that way, then a probe from the host; then the probes that way after a poison from the host."""
    import torch
    bf.check_poison()
    s = mse.Searcher(bf.device())

    def dev_call(parts, k):
        q = bf.queries((parts,))
        nq = len(q)
        buf = torch.zeros(nq * D + 8, dtype=torch.int16, device="cuda")
        qd = buf[1:1 + nq * D]
        qd.copy_(torch.from_numpy(q.view(np.int16).reshape(-1)))
        assert qd.data_ptr() % 16 == 2
        out_s = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        out_i = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.bruteforce_topk_dev(qd.data_ptr(), nq, k, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)
        mse.ffi.check(mse.ffi.lib().mse_device_synchronize())
        ws, wi = bf.want((parts,), k)
        assert np.array_equal(out_i.cpu().numpy().view(np.uint32), wi) and np.array_equal(out_s.cpu().numpy(), ws), (parts, k)

    dev_call((P, 0, 40), 100)
    run_sequence(bf, [step((Q, 0, 3), 10)], searcher=s)
    dev_call((P, 0, 320), 10)
    run_sequence(bf, [step((Q, 0, 1), 10, mode="exact")], searcher=s)
    run_sequence(bf, [step((P, 0, 330), 100)], searcher=s)
    dev_call((Q, 0, 9), 10)
    dev_call((Q, 0, 300), 1)
    s.close()


def test_two_searchers_over_one_base(gpu, bf, mse):
    """two Searchers over one VectorList share its norm cache and dispatcher and nothing else: poison on one, probe on the other, in turn"""
    vl = bf.device()
    a, b = mse.Searcher(vl), mse.Searcher(vl)
    turns = [(a, step((P, 0, 320), 100)), (b, step((Q, 0, 3), 10)), (a, step((Q, 0, 9), 10)),
             (b, step((P, 0, 330), 10)), (a, step((P, 0, 40), 1000)), (b, step((Q, 0, 130), 1)),
             (a, step((Q, 0, 2), 3, mode="exact")), (b, step((T, 0, 12), 10, widened=True)), (a, step((T, 0, 12), 10, widened=True)),
             (b, step((Q, 0, 5), 10, widened=False)), (a, step((Q, 0, 40), 32, allow="seventeen"))]
    for s, st in turns:
        run_sequence(bf, [st], searcher=s)
    a.close()
    b.close()


# ---- ScalarQuantizerIndex: search between adds ----------------------------------------------------------------------------------------

FAMILIES = 8


def _family_rows(f):
    """where family f sits among the 3000 rows (which start at row 1024, a group boundary): row f of the first 60 32-row groups"""
    return 32 * np.arange(60) + f


def _index_rows(orc, d, rng):
    """what is added, in order: 1000 rows of norm ~ 0.01; 24 rows of norm ~ 1, 20 of them one-ulp neighbours of one row; 3000 rows,
    among them 8 families of 60 near-copies of one row, one copy per 32-row group.
    A family is searched with its own query q of norm 200; its row is a + q / 2 with a of norm 200 orthogonal to q: a score of 20000,
    above every other row's, under which products of about 30000 cancel.  A copy differs from the row in three coordinates by one f16
    ulp, where that moves the score by about two f32 ulps: 60 near-ties in 60 groups where the first round takes 16, so the query is
    certified only after the widening (eps ~ 12 under the true norm bound).
    Measured once on an MI355X: the matrix-core sum of such a row is within 5 ulps of the reference-order sum and moves WITH it from
    copy to copy (spread 1-2 ulps), so the 16 nominated groups held the best 7 copies in 15 of 16 families, and in the other one the
    k-th score did not clear the 16th group key.  A norm bound left at the first add's value (eps 6e-4) therefore returns the same
    answers on this data: that mutation is NOT caught here -- the bound guards against rows the scan misorders, and near-copies
    are not such rows."""
    small = (0.01 * rng.standard_normal((1000, d)) / np.sqrt(d)).astype(np.float32)
    big = (rng.standard_normal((24, d)) / np.sqrt(d)).astype(np.float32)
    proto = big[2].copy()
    near = np.tile(proto, (20, 1))
    near[np.arange(20), rng.integers(0, d, 20)] *= np.float32(1.0 + 2.0 ** -9)      # one-ulp-ish perturbations of one row
    big[4:] = near
    more = (rng.standard_normal((3000, d)) / np.sqrt(d)).astype(np.float32)
    heads = (200.0 * rng.standard_normal((FAMILIES, d)) / np.sqrt(d)).astype(np.float16)
    for f, head in enumerate(heads):
        h = head.astype(np.float64)
        a = rng.standard_normal(d)
        a -= (a @ h) / (h @ h) * h
        row = (a * (200.0 / np.linalg.norm(a)) + 0.5 * h).astype(np.float16)
        ulp = float(np.spacing(np.float32(row.astype(np.float64) @ h)))
        move = np.abs(h) * np.spacing(np.abs(row)).astype(np.float64) / ulp             # of the score, in ulps, by one f16 ulp of a coordinate
        coords = np.argsort(np.abs(np.log2(np.maximum(move, 1e-9) / 2.0)))[:16]
        copies = np.tile(row, (60, 1))
        for c in copies:                                                             # three coordinates, up or down: distinct rows
            at = rng.choice(coords, 3, replace=False)
            c[at] = np.nextafter(c[at], (np.inf * rng.choice([-1.0, 1.0], 3)).astype(np.float16))
        more[_family_rows(f)] = copies.astype(np.float32)
    return small, big, more, proto, heads.astype(np.float32)


@pytest.mark.parametrize("d", [128, 1152])
def test_index_search_between_adds(gpu, mse, orc, d):
    """One index, searched after every add: the row block is re-allocated when it outgrows 1024 rows, and the row-norm bound behind the
    matrix-core certificate follows every add -- the second add raises it a hundredfold and brings 20 near-copies of one row, the third
    raises it again and brings families of near-copies spread over 60 groups each, which are in order only after the widening.
    Labels and distances equal the oracle's over the rows added so far, and a fresh index's that got the same rows in one add."""
    rng = np.random.default_rng(1000 + d)
    small, big, more, proto, heads = _index_rows(orc, d, rng)
    q = rng.standard_normal((300, d)).astype(np.float32)
    q[3] = proto * np.float32(7.0)                                            # the row the near-copies surround
    fam = np.concatenate([q[:3], heads])                                      # 11 queries (the matrix-core pass), 8 of them family rows
    idx = mse.ScalarQuantizerIndex(d)
    added = np.empty((0, d), np.float32)

    def add(x):
        nonlocal added
        idx.add(x)
        added = np.concatenate([added, x])
        assert idx.ntotal() == len(added)

    def search(qs, k, allow=None, over=None):
        """the long-lived index == the oracle over the rows so far (or the filter's rows `over`) == a fresh index filled in one add"""
        codes = orc.f16_bits(added)
        res = idx.search(qs, k, allow=allow)
        if over is None:
            wd, wl = orc.index_search(codes, qs, k, order=0)
        else:
            wd, wl = orc.index_search(codes[over], qs, k, order=0)
            wl = np.where(wl >= 0, over[np.maximum(wl, 0)], -1)
        assert np.array_equal(res.labels, wl) and np.array_equal(res.distances, wd), (len(added), len(qs), k)
        if allow is None:
            fresh = mse.ScalarQuantizerIndex(d)
            fresh.add(added)
            fr = fresh.search(qs, k)
            fresh.close()
            assert np.array_equal(fr.labels, wl) and np.array_equal(fr.distances, wd), ("fresh", len(added), len(qs), k)
        return res

    add(small)                                                                # 1
    search(q[:11], 7)                                                         # 2: the matrix-core pass under the small norm bound
    add(big)                                                                  # 3: past 1024 rows; norms a hundred times larger
    res = search(q[:11], 7)                                                   # 4
    assert np.all(res.labels[3] >= 1000)                                      # (the near-copies are what query 3 finds)
    search(q, 7)                                                              # 5: 300 queries
    search(q[3:4], 1)                                                         # 6: the exact pass
    before = mse.RowFilter(rng.random(len(added)) < 0.5)
    over = np.flatnonzero(before.to_mask())
    add(more)                                                                 # 7
    search(q[:9], 100)                                                        # 8
    res = search(fam, 7)                                                      # ... and the families: 60 near-ties in 60 groups each
    for f in range(FAMILIES):
        assert np.all(np.isin(res.labels[3 + f], 1024 + _family_rows(f))), f
    search(q[:9], 100, allow=before, over=over)                               # 9: a filter from before the last add: its rows only
    search(q[:11], 7, allow=before, over=over)
    search(q[:2], 3)
    before.close()
    idx.close()
    # 10: k above ntotal right after the first add of a second index
    five = mse.ScalarQuantizerIndex(d)
    five.add(more[:5])
    res = five.search(q[:11], 9)
    wd, wl = orc.index_search(orc.f16_bits(more[:5]), q[:11], 9, order=0)
    assert np.array_equal(res.labels, wl) and np.array_equal(res.distances, wd)
    assert np.all(res.labels[:, 5:] == -1) and np.all(res.distances[:, 5:] == -np.finfo(np.float32).max)
    five.close()


# ---- graph search scratch (pool[16]) ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ix(gpu, orc, mse):
    from test_gpu_beam_envelope import Index
    return Index(orc, mse)


def _same(a, b, where):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for key in a:
            _same(a[key], b[key], (where, key))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for n, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (where, n))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), where


def _valid(res):
    """a padded disk_search_batch result cut to what each query wrote (the tails of the host arrays are not written)"""
    from test_gpu_beam_envelope import row
    return [row(res, i) for i in range(res["buf_len"].shape[0])]


def test_graph_search_scratch_between_shapes(ix, mse, orc):
    """One Searcher through graph searches of very different shapes, a six-query call after each: 1100 exactly scored queries at
    L = 40; 24 ADC-scored queries with bias at L = 1024; the request path with de-duplication on, then off; f32 queries, then f16.
    Every call equals the same single call on a fresh Searcher -- buffers, visited records, counters -- and the six-query calls the
    oracle (the envelope file pins the oracle parity of the large shapes; the order is what is new here)."""
    from test_gpu_beam_envelope import CASES, N as NROWS, SCALES, check_case
    vl = mse.VectorList.from_f16s(ix.base, D)
    s = mse.Searcher(vl)
    small = CASES[0]                                                            # 6 queries, ADC with bias, beam 8 x degree 64, L = 65
    small_exact = (8, 64, False, True, 65, 6, 1)

    def batch(searcher, case, f32=False):
        beam, md, adc, bias, L, nq, seed = case
        adj, degs, dg, qh, luts, starts, scales, disable_pq = ix.inputs(case)
        if f32:
            return mse.disk_search_batch(searcher, ix.gpq, ix.gcodes, dg, starts, ix.queries(nq, seed)[0], None, scales, disable_pq, beam,
                                         search_list=L, visited_cap=NROWS, as_arrays=True)
        return mse.disk_search_batch(searcher, ix.gpq, ix.gcodes, dg, starts, qh, luts, scales, disable_pq, beam, search_list=L,
                                     visited_cap=NROWS, as_arrays=True)

    def topk(searcher, case, k, f32=False):
        beam, md, adc, bias, L, nq, seed = case
        adj, degs, dg, qh, luts, starts, scales, disable_pq = ix.inputs(case)
        if f32:
            return mse.disk_query_topk(searcher, ix.gpq, ix.gcodes, dg, ix.queries(nq, seed)[0], k, starts, None, scales, disable_pq, beam, L)
        return mse.disk_query_topk(searcher, ix.gpq, ix.gcodes, dg, qh, k, starts, luts, scales, disable_pq, beam, L)

    def both(fn, *args, **kw):
        got = fn(s, *args, **kw)
        fresh = mse.Searcher(vl)
        want = fn(fresh, *args, **kw)
        fresh.close()
        if fn is batch:
            _same(_valid(got), _valid(want), (args, kw))
        else:
            _same(got, want, (args, kw))
        return got

    def six():
        check_case(ix, small, res=both(batch, small))
        check_case(ix, small_exact, res=both(batch, small_exact))

    six()
    both(batch, (2, 64, False, True, 40, 1100, 21))                             # 1100 queries, exact scoring, L = 40
    six()
    both(batch, (8, 128, True, True, 1024, 24, 22))                             # 24 queries, ADC with bias, L = 1024
    six()
    dg = ix.graph(64)[2]
    try:
        mse.set_dedup(dg, mse.DUPLICATES_THRESHOLD)
        both(topk, (8, 64, True, True, 300, 24, 23), 500)
        both(topk, small, 10)
        mse.set_dedup(dg, 0.0)
        both(topk, (8, 64, True, True, 300, 24, 23), 500)
        ids, scores, stats = both(topk, small, 10)
    finally:
        mse.set_dedup(dg, 0.0)
    for i in range(6):                                                          # the request path of the six-query call against the oracle
        _, _, ovids, ovsc, ocm, opc = ix.want(small, i)
        order = sorted(range(len(ovids)), key=lambda j: (-int(ovsc[j]), int(ovids[j])))[:10]
        m = len(order)
        assert np.array_equal(ids[i, :m], ovids[order]) and np.array_equal(scores[i, :m], ovsc[order]), i
        assert np.all(ids[i, m:] == ID_NONE) and np.all(scores[i, m:] == I64_MIN), i
        assert (int(stats["cmps"][i]), int(stats["pq_cmps"][i]), int(stats["n_visited"][i])) == (ocm, opc, len(ovids)), i
    six()
    both(batch, (8, 64, True, True, 200, 40, 24), f32=True)                     # f32 queries: f16 copies and tables made on the device
    six()
    both(batch, (8, 64, True, True, 200, 40, 24))                               # the same queries as f16 rows with the oracle's tables
    both(topk, small, 10, f32=True)
    six()
    s.close()
    vl.close()
