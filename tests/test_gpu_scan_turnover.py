"""The 320-query search kernel's epilogue (scan_mfma.hip scan_mfma2d_kernel, GR = 64): the maximum over a wave's 64 rows is formed in
registers and TRANSPOSED -- after two rounds of row exchanges lane (i, g) of a wave holds the finished maxima of column i of the column
tiles g, 4 + g and 8 + g of its 160 columns, and writes or appends those.  A wrong row or column-tile map moves a group maximum to
another column or loses it, so the cases plant, for every query, one row far above all others at a chosen position of a 64-row group
and want the oracle's ids and i64 scores (orc.bruteforce_topk) from the thresholded form (forced, stride 3: tiles 0, 3, 6 are the sample)
and from the dense form (off).
Shapes: 7 whole tiles (1 792 rows) plus tails of 0, 1, 63, 65 and 255 rows (a ragged eighth tile with one to four groups); 257 queries
(63 zero-padded columns) and 320; k = 1 and 10."""
import functools

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152
TILES = 7
STRIDE = 3


@functools.lru_cache(maxsize=None)
def _rows(seed, stream, n):
    from oracle import orc
    a = orc.gen_rows_f16(seed, stream, n)
    a.setflags(write=False)
    return a


def _both_forms(mse, base, q, k, want):
    """the thresholded and the dense form against the oracle's answer; returns the statistics of the thresholded call"""
    s = mse.Searcher(mse.VectorList.from_f16s(base, D))
    s.set_sparse_maxima("forced", STRIDE)
    ss, si = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    st = s.last_stats()
    print("forced sparse:", st)
    s.set_sparse_maxima("off")
    ds, di = s.bruteforce_topk(q, k, mse.MODE_MFMA)
    assert s.last_stats()["sparse_passes"] == 0
    s.close()
    assert np.array_equal(si, want[1]) and np.array_equal(ss, want[0]), "the thresholded form differs from the oracle"
    assert np.array_equal(di, want[1]) and np.array_equal(ds, want[0]), "the dense form differs from the oracle"
    assert st["sparse_passes"] > 0 and st["sparse_fallbacks"] == 0, st
    return st


@functools.lru_cache(maxsize=None)
def _planted(tail, nq):
    """base of n rows in which row 64 G(c) + p(c) is a copy of query c; G runs over all groups, p over all 64 positions of a group"""
    n = TILES * 256 + tail
    base = _rows(SEED_BASE, 53, n).copy()
    q = _rows(SEED_QUERY, 53, 320)[:nq]
    n_groups = (n + 63) // 64
    at = np.empty(nq, np.int64)
    taken = set()
    for c in range(nq):
        g, p = c % n_groups, (11 * c + c // 64) % 64
        while 64 * g + p >= n or 64 * g + p in taken:   # a ragged last group, or the position already holds a winner
            p = (p + 1) % 64
            if p == 0:
                g = (g + 1) % n_groups
        at[c] = 64 * g + p
        taken.add(int(at[c]))
    base[at] = q
    base.setflags(write=False)
    # the case is what it says: all 64 row positions, and in each of the 2 x 10 column tiles winners in all four 16-row blocks of a wave
    assert len(set(int(r) % 64 for r in at)) == 64
    for t in range((nq + 15) // 16):
        assert len(set((int(r) % 64) // 16 for r in at[16 * t:16 * t + 16])) == 4 or t == nq // 16
    return base, q, at


@functools.lru_cache(maxsize=None)
def _planted_oracle(tail, nq, k):
    from oracle import orc
    base, q, at = _planted(tail, nq)
    ws, wi = orc.bruteforce_topk(base, q, k)
    assert np.array_equal(wi[:, 0], at.astype(np.uint32)), "a planted row is not its query's best row"
    # ... and every other row scores well below: the second best has less than half the winner's score
    if k > 1:
        assert (ws[:, 1] * 2 < ws[:, 0]).all()
    return ws, wi


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("nq", [257, 320])
@pytest.mark.parametrize("tail", [0, 1, 63, 65, 255])
def test_planted_winners(gpu, mse, orc, tail, nq, k):
    base, q, _ = _planted(tail, nq)
    _both_forms(mse, base, q, k, _planted_oracle(tail, nq, k))


# Lane (i, g) of query half h speaks for columns 160 h + 16 (g + 4 j) + i, j = 0 .. 2 (j = 2: g < 2 only).  Copies of all the queries of
# such a lane sit in the SAME 64-row groups of tiles the sample does not see (tiles 1, 2, 4 with stride 3), three groups per lane: every
# one of these queries has three groups above its threshold, and in each of them all the registers of the lane append in one tile.
@pytest.mark.parametrize("nq", [257, 320])
def test_all_registers_of_a_lane_append_in_one_tile(gpu, mse, orc, nq):
    n = TILES * 256 + 65
    base = _rows(SEED_BASE, 59, n).copy()
    q = _rows(SEED_QUERY, 59, 320)[:nq]
    lanes = [(0, 0, 3), (0, 1, 15), (1, 0, 0), (1, 1, 9), (0, 2, 7), (0, 3, 12), (1, 3, 5)]   # (h, g, i)
    groups = [(1, 0), (2, 3), (4, 2)]   # (tile, row group of the tile): three groups per lane, shifted per lane below
    planted = {}
    for li, (h, g, i) in enumerate(lanes):
        cols = [160 * h + 16 * (g + 4 * j) + i for j in range(3) if g + 4 * j < 10]
        cols = [c for c in cols if c < nq]
        for gi, (tile, rg) in enumerate(groups):
            grp = tile * 4 + (rg + li) % 4
            for j, c in enumerate(cols):
                row = 64 * grp + (5 * li + 17 * gi + 23 * j) % 64
                while row in planted:
                    row = 64 * grp + (row + 1) % 64
                planted[row] = c
    for row, c in planted.items():
        base[row] = q[c]
    ws, wi = orc.bruteforce_topk(base, q, 10)
    for row, c in planted.items():   # the case is what it says: every copy is among its query's three best rows
        assert row in wi[c, :3]
    st = _both_forms(mse, base, q, 10, (ws, wi))
    assert st["sparse_longest_list"] >= 3


# Rows with only positive and queries with only negative components: every score, so every group maximum and every threshold, is below
# zero.  An accumulator that starts from anything but zero, a zero or a threshold taken for a maximum would be the largest value there is.
@pytest.mark.parametrize("nq", [257, 320])
def test_negative_scores(gpu, mse, orc, nq):
    n = TILES * 256 + 63
    base = _rows(SEED_BASE, 61, n) & np.uint16(0x7FFF)
    q = _rows(SEED_QUERY, 61, 320)[:nq] | np.uint16(0x8000)
    ws, wi = orc.bruteforce_topk(base, q, 10)
    assert (ws < 0).all()
    _both_forms(mse, np.ascontiguousarray(base), np.ascontiguousarray(q), 10, (ws, wi))
