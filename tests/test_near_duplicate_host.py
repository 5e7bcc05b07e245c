"""The restatement the GPU tests of the near-duplicate join compare against (tests/near_duplicate_ref.py), on hand-written cases, and the
binding of the new symbols.  No device is needed."""
import ctypes as C

import numpy as np

import near_duplicate_ref as ref

NONE = ref.NONE


def matrix(n, edges, hit=95, miss=10):
    s = np.full((n, n), miss, np.int64)
    for a, b in edges:
        s[a, b] = s[b, a] = hit
    np.fill_diagonal(s, 100)
    return s


def test_triangle_keeps_the_third_row():
    """a ~ b ~ c with a !~ c: b is dropped by a, and c -- whose only earlier neighbour is dropped -- is kept.  Under an "any earlier row"
    rule c would be dropped too."""
    lo, hi, sc = ref.pairs_from_scores(matrix(3, [(0, 1), (1, 2)]), 90)
    assert lo.tolist() == [0, 1] and hi.tolist() == [1, 2] and sc.tolist() == [95, 95]
    kept, rep = ref.keep_first(3, lo, hi)
    assert kept.tolist() == [True, False, True] and rep.tolist() == [0, 0, 2]
    assert ref.labels(kept, rep).tolist() == [0, 0, NONE]


def test_alternating_path():
    n = 9
    lo, hi, _ = ref.pairs_from_scores(matrix(n, [(i, i + 1) for i in range(n - 1)]), 90)
    kept, rep = ref.keep_first(n, lo, hi)
    assert kept.tolist() == [i % 2 == 0 for i in range(n)]
    assert rep.tolist() == [i - i % 2 for i in range(n)]
    assert ref.labels(kept, rep).tolist() == [0, 0, 2, 2, 4, 4, 6, 6, NONE]


def test_canonical_order_and_lowest_kept_neighbour():
    """row 4 pairs with 1, 2 and 3; 1 is dropped by 0, so its representative is 2, the lowest KEPT earlier neighbour"""
    lo, hi, _ = ref.pairs_from_scores(matrix(5, [(0, 1), (1, 4), (2, 4), (3, 4)]), 90)
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 1), (1, 4), (2, 4), (3, 4)]
    kept, rep = ref.keep_first(5, lo, hi)
    assert kept.tolist() == [True, False, True, True, False] and rep.tolist() == [0, 0, 2, 3, 2]
    assert ref.labels(kept, rep).tolist() == [0, 0, 2, NONE, 2]


def test_excluded_row_is_in_no_pair():
    s = matrix(4, [(0, 1), (1, 2), (2, 3)])
    within = np.array([True, False, True, True])
    lo, hi, _ = ref.pairs_from_scores(s, 90, within=within)
    assert list(zip(lo.tolist(), hi.tolist())) == [(2, 3)]
    kept, rep = ref.keep_first(4, lo, hi)
    assert kept.tolist() == [True, True, True, False]      # the excluded row comes out kept ...
    assert ref.labels(kept, rep).tolist() == [NONE, NONE, 2, 2]   # ... and ungrouped
    lo, hi, _ = ref.pairs_from_scores(s, 90, within=within[:2])   # a filter shorter than the base excludes the later rows
    assert lo.size == 0


def test_window_cuts_a_pair():
    s = matrix(8, [(0, 3), (1, 5), (6, 7)])
    got = lambda w: list(zip(*[a.tolist() for a in ref.pairs_from_scores(s, 90, window=w)[:2]]))
    assert got(0) == [(0, 3), (1, 5), (6, 7)]
    assert got(4) == [(0, 3), (1, 5), (6, 7)]
    assert got(3) == [(0, 3), (6, 7)]        # distance exactly the window stays, window + 1 goes
    assert got(1) == [(6, 7)]


def test_threshold_is_inclusive():
    s = matrix(2, [(0, 1)])
    assert ref.pairs_from_scores(s, 95)[0].size == 1 and ref.pairs_from_scores(s, 96)[0].size == 0


def test_new_symbols_are_bound(mse):
    from mse import ffi
    vp, sz, u32p, i64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    want = {
        "mse_join_self": (vp, [vp, C.c_int64, C.c_uint64, vp, C.c_int, C.c_uint64]),
        "mse_pairs_free": (None, [vp]),
        "mse_pairs_rows": (sz, [vp]),
        "mse_pairs_count": (sz, [vp]),
        "mse_pairs_read": (C.c_int, [vp, sz, sz, u32p, u32p, i64p]),
        "mse_join_stats": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "mse_debug_join_candidate_capacity": (C.c_int, [vp, C.c_uint64]),
        "mse_pairs_duplicates": (vp, [vp]),
        "mse_pairs_groups": (vp, [vp]),
        "mse_pairs_representatives": (C.c_int, [vp, u32p]),
    }
    for name, sig in want.items():
        assert ffi.SIGNATURES.get(name) == sig, name
        assert hasattr(C.CDLL(ffi.LIB_PATH), name), name
    assert hasattr(mse, "RowPairs") and hasattr(mse.Searcher, "near_duplicates") and hasattr(mse.DeviceGraph, "near_duplicates")
