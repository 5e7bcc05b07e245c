"""The row ring of the 320-query scan kernel (scan_mfma.hip scan_mfma2d_kernel, S = 2): which K block of which row a stage holds when it
is read.  A stage that is read stale or half written corrupts ONE K block of some rows, and the exact re-score repairs a wrong nomination
score unless enough other groups outrank it, so these cases are built to notice one wrong K block in one row:
  - per query one WINNER row that equals the query (unit norm: exact score 1).  With K block b replaced by what the stage held before
    (block b - 2 of the row, or a block of the tile the workgroup ran before) its matrix-core score falls to about 1 - 1 / (d / 64);
  - per guarded query DECOY rows, one in each of up to 80 other 64-row groups -- more than the widening takes in, 4 * max(k + 8, 16) = 72:
    the query scaled by 0.97, 0.9695, 0.969, ... (steps of 0.0005).  The steps are the one departure from "all decoys at 0.97": equal
    decoys tie with each other, no round certifies against a tie, and the query ends in the exact-order fallback, which returns the right
    answer whatever the scan did.  Steps of 0.0005 are about two of the certificate's eps (2.8e-4), so a healthy scan certifies in its
    first round (k = 10: the tenth score 0.966 against the best group left out, 0.9615), and a winner corrupted down to 0.944 (d = 1152) or
    0.5 (d = 128) lies below the 18 groups of the first round, whose answer then certifies WRONGLY: decoys where the winner should be;
  - every other row comes from the generator and scores below 0.2 at d = 1152 (below 0.6 at d = 128 and 256), which the cases assert.
Expected ids and i64 scores: orc.bruteforce_topk over the whole base where it is small, over the planted rows where it is large.
Winner positions: both halves of a 64-row group (rows 0-31 are fetched by one wave of the pair, 32-63 by the other), all four row groups
of a tile, the first, a middle and the last tile of a workgroup.
Shapes: d = 1152 (18 K blocks) and the smallest even K-block counts the 320-query path takes, d = 128 (2: every prefetch crosses a tile
boundary) and 256 (4) -- the launchers accept both; bases of 1, 63, 64, 65, 255, 256, 257 rows; 7 tiles plus 0, 1, 65, 255 rows; one base
of 2 CUs + 3 tiles plus 65 rows (every workgroup runs two or three tiles, the last one ragged).
Forms: dense, thresholded (forced, stride 3), masked (a filter that allows every planted row); 257 and 320 queries; k = 1 and 10.
Checked once against a build that fetched K block 5 in place of block 7 for rows 0-31 of row group 1 (one stale block, as a ring off by
one stage leaves it): 63 of the 169 cases fail, every d = 1152 case from seven tiles on, the unplanted one among them; the bases of at
most 257 rows cannot see it (all their groups are re-scored) and are here for the clamped and ragged paths."""
import functools

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
TILES = 7
STRIDE = 3
N_DECOYS = 80
TOP, STEP = 0.97, 0.0005
FORMS = ["dense", "thresholded", "masked"]


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _queries(d):
    from oracle import orc
    q = orc.gen_rows_f16(SEED_QUERY, 71, 320, d)
    q.setflags(write=False)
    return q


def _plant(n, d, winners, guarded):
    """Generator rows with row winners[c] = query c and, for each guarded query, decoys in other groups.  Returns the base, the sorted
    ids of the planted rows and {c: [decoy rows, best first]}."""
    from oracle import orc
    base = orc.gen_rows_f16(SEED_BASE, 71, n, d)
    q = _queries(d)
    n_groups = (n + 63) // 64
    taken = set(int(r) for r in winners.values())
    assert len(taken) == len(winners)
    for c, r in winners.items():
        base[r] = q[c]
    decoys = {}
    for c in guarded:
        q32 = orc.f16_to_f32(q[c])
        own = winners[c] // 64
        rows = []
        for step in range(1, n_groups):
            if len(rows) == N_DECOYS:
                break
            g = (own + step * 37) % n_groups if n_groups % 37 else (own + step) % n_groups
            for t in range(64):   # a free row of the group (a ragged last group may have none)
                r = 64 * g + (7 * c + len(rows) + t) % 64
                if r < n and r not in taken:
                    base[r] = orc.f16_bits(q32 * np.float32(TOP - STEP * len(rows)))
                    taken.add(r)
                    rows.append(r)
                    break
        decoys[c] = rows
        assert len(set(r // 64 for r in rows)) == len(rows) and own not in set(r // 64 for r in rows)
    base.setflags(write=False)
    return base, np.array(sorted(taken), np.int64), decoys


def _others_below(base, planted, d, bound):
    """every row that was not planted scores below `bound` with every query (float32 products: the margin to the decoys is 0.3 and more)"""
    q32 = _queries(d).view(np.float16).astype(np.float32).T
    keep = np.ones(len(base), bool)
    keep[planted] = False
    worst = -1.0
    for lo in range(0, len(base), 8192):
        rows = base[lo:lo + 8192][keep[lo:lo + 8192]]
        if len(rows):
            worst = max(worst, float((rows.view(np.float16).astype(np.float32) @ q32).max()))
    assert worst < bound, worst
    return worst


class Case:
    """a planted base on the device with its searcher, its filter, and the oracle's answers per (form, nq, k)"""

    def __init__(self, mse, n, d, winners, guarded, whole):
        from oracle import orc
        self.mse, self.orc, self.n, self.d, self.whole = mse, orc, n, d, whole
        self.base, self.planted, self.decoys = _plant(n, d, winners, guarded)
        self.winners = winners
        if whole:
            self.sub = np.arange(n, dtype=np.int64)
        else:   # the answers come from the planted rows alone: nothing else comes near them
            _others_below(self.base, self.planted, d, 0.2 if d == 1152 else 0.6)
            self.sub = self.planted
        # the filter: every planted row, and four of five others
        allow = np.arange(n) % 5 != 2
        allow[self.planted] = True
        self.allow = allow
        self.searcher = mse.Searcher(mse.VectorList.from_f16s(self.base, d))
        self.filter = mse.RowFilter(allow)
        self.answers = {}

    def want(self, masked, nq, k):
        key = (masked and self.whole, nq, k)
        if key not in self.answers:
            rows = self.sub[self.allow[self.sub]] if masked else self.sub
            ws, wi = self.orc.bruteforce_topk(np.ascontiguousarray(self.base[rows]), _queries(self.d)[:nq], k)
            wi = rows[wi].astype(np.uint32)
            for c, r in self.winners.items():   # the case is what it says: the winner is its query's best row, the decoys follow in order
                if c < nq:
                    assert wi[c, 0] == r, (c, r, wi[c])
                    if c in self.decoys and k > 1:
                        m = min(k - 1, len(self.decoys[c]))
                        assert list(wi[c, 1:1 + m]) == self.decoys[c][:m], (c, wi[c], self.decoys[c][:m])
            if not self.whole:   # ... and planted rows fill the whole answer: what was left out of the oracle's rows cannot be in it
                assert all(len(self.decoys[c]) >= k - 1 for c in range(nq))
            self.answers[key] = (ws, wi)
        return self.answers[key]

    def check(self, form, nq, k):
        mse, s = self.mse, self.searcher
        k = min(k, int(self.allow.sum()) if form == "masked" else self.n)
        q = _queries(self.d)[:nq]
        ws, wi = self.want(form == "masked", nq, k)
        if form == "thresholded":
            s.set_sparse_maxima("forced", STRIDE)
        else:
            s.set_sparse_maxima("off")
        gs, gi = s.bruteforce_topk(q, k, mse.MODE_MFMA, allow=self.filter if form == "masked" else None)
        st = s.last_stats()
        print(form, nq, k, st)
        bad = np.flatnonzero((gi != wi).any(axis=1) | (gs != ws).any(axis=1))
        assert bad.size == 0, f"{form}: queries {bad[:8]} differ, e.g. got {gi[bad[0]]} want {wi[bad[0]]}"
        # the tile-subset form ran wherever the sample (every third tile) holds k groups, and no list overflowed (fewer groups than slots)
        n_tiles, n_a = (self.n + 255) // 256, ((self.n + 255) // 256 + STRIDE - 1) // STRIDE
        n_sample = (n_a - 1) * 4 + min(4, (self.n + 63) // 64 - (n_a - 1) * STRIDE * 4)
        if form == "thresholded" and n_tiles >= 2 and n_sample >= k:
            assert st["sparse_passes"] > 0 and st["sparse_fallbacks"] == 0, st


_CASES = {}


def _case(mse, key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ---- one tile and less: 1 .. 257 rows (row clamping, one or two tiles, the two blocks fetched behind the last tile) -------------------
def _tiny(mse, n):
    winners = {c: (n - 1 - 5 * c) % n for c in range(min(320, (n + 4) // 5))}   # distinct rows, the last row among them
    return Case(mse, n, 1152, winners, [], True)


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_small_bases(gpu, mse, orc, n, form, nq, k):
    _case(mse, ("tiny", n), lambda: _tiny(mse, n)).check(form, nq, k)


# ---- seven tiles and a tail: every query has a winner, 24 guarded ones cover (tile 0 | 3 | last) x row group x half ------------------
def _seven(mse, tail):
    n = TILES * 256 + tail
    n_groups = (n + 63) // 64
    last = (n - 1) // 256
    winners, guarded = {}, []
    for gi in range(24):
        c = gi * 13 + (gi % 2)          # 0 .. 300: both query halves, the columns past 256 among them
        tile, rg, half = [0, 3, last][gi % 3], (gi // 3) % 4, gi // 12
        r = 256 * tile + 64 * rg + 32 * half + (5 * gi) % 32
        if r >= n:                      # the ragged tile has no such row: the last whole tile then
            r -= 256 * (tile - (TILES - 1))
        winners[c] = r
        guarded.append(c)
    if tail:   # the base's very last row is a guarded winner too
        winners[guarded[2]] = n - 1
    taken = set(winners.values())
    assert len(taken) == 24
    for c in range(320):
        if c in winners:
            continue
        g, p = c % n_groups, (11 * c + c // 64) % 64
        while 64 * g + p >= n or 64 * g + p in taken:
            p = (p + 1) % 64
            if p == 0:
                g = (g + 1) % n_groups
        winners[c] = 64 * g + p
        taken.add(64 * g + p)
    case = Case(mse, n, 1152, winners, guarded, True)
    rows = [winners[c] for c in guarded]
    assert {r % 64 // 32 for r in rows} == {0, 1} and {r % 256 // 64 for r in rows} == {0, 1, 2, 3}
    assert {0, 3} <= {r // 256 for r in rows} and max(r // 256 for r in rows) == last
    assert all(len(case.decoys[c]) >= 18 for c in guarded)   # more decoy groups than the first round re-scores
    return case


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tail", [0, 1, 65, 255])
def test_seven_tiles_and_a_tail(gpu, mse, orc, tail, form, nq, k):
    _case(mse, ("seven", tail), lambda: _seven(mse, tail)).check(form, nq, k)


# ---- 2 CUs + 3 tiles and 65 rows: every workgroup runs two or three tiles, the base's last tile is ragged; every query is guarded ------
def _large_rows():
    return (2 * _n_cu() + 3) * 256 + 65


def _large(mse, d):
    cu = _n_cu()
    n = _large_rows()
    wgs = [0, 1, 2, 3, 5, cu // 2, cu - 1]   # workgroups 0 .. 2 run three whole tiles, 3 ends in the ragged one, the others run two
    winners = {}
    taken = set()
    for c in range(320):
        wg = wgs[c % 7]
        slot = (c // 7) % 3                   # first, middle, last tile of the workgroup in the dense form
        tile = wg + cu * slot
        if tile * 256 >= n:                   # the workgroup has two tiles only
            tile = wg + cu
        rg, half = (c // 21) % 4, (c // 84) % 2
        r = 256 * tile + 64 * rg + 32 * half + (11 * c) % 32
        while r >= n or r in taken:           # the ragged tile: rows 0 .. 64 only
            r = 256 * tile + (r - 256 * tile + 1) % (min(256, n - 256 * tile))
        winners[c] = r
        taken.add(r)
    case = Case(mse, n, d, winners, list(range(320)), False)
    rows = np.array([winners[c] for c in range(320)])
    assert set(rows % 64 // 32) == {0, 1} and set(rows % 256 // 64) == {0, 1, 2, 3}
    tiles = set(int(t) for t in rows // 256)
    assert {0, cu, 2 * cu, 3, 3 + cu, 3 + 2 * cu, cu - 1, 2 * cu - 1} <= tiles   # first, middle, last; the ragged tile; a two-tile workgroup
    assert all(len(v) == N_DECOYS for v in case.decoys.values())
    return case


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("d", [1152, 128, 256])
def test_two_and_three_tiles_per_workgroup(gpu, mse, orc, d, form, nq, k):
    assert mse.ffi.lib().mse_queries_per_pass_max(d) == 320   # an even K-block count: the 320-query kernel takes this width
    _case(mse, ("large", d), lambda: _large(mse, d)).check(form, nq, k)


# ---- without planting: generator rows, where a tenth-best row is one of thousands of near equals ---------------------------------------
def test_large_base_equals_the_exact_order_mode(gpu, mse, orc):
    n = _large_rows()
    vecs = mse.VectorList.generate(SEED_BASE, 0, n)
    q = orc.gen_rows_f16(SEED_QUERY, 73, 320)
    s = mse.Searcher(vecs)
    es, ei = s.bruteforce_topk(q, 10, mse.MODE_EXACT)
    for form in ("off", "forced"):
        s.set_sparse_maxima(form, STRIDE)
        ms, mi = s.bruteforce_topk(q, 10, mse.MODE_MFMA)
        print(form, s.last_stats())
        assert np.array_equal(mi, ei) and np.array_equal(ms, es), form
    s.close()
