"""The restatement the GPU tests of the cross join compare against (tests/cross_join_ref.py), on hand-written cases, and the binding of the
new symbols.  No device is needed."""
import ctypes as C

import numpy as np

import cross_join_ref as ref

NONE = ref.NONE


def lists(pairs):
    a = np.array(sorted(pairs), np.int64).reshape(-1, 2)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32)


def run(m, cross, among):
    """cross: (incoming row, base row) pairs; among: (lo, hi) pairs of incoming rows or None -> the walk, checked against the rounds"""
    ch, cl = lists(cross)
    al, ah = (None, None) if among is None else lists(among)
    kept, rb, ri = ref.admit(m, ch, cl, al, ah)
    rounds, kept_by_rounds = ref.admit_rounds(m, ch, al, ah)
    assert np.array_equal(kept, kept_by_rounds), "the rounds resolve the walk"
    return kept.tolist(), rb.tolist(), ri.tolist(), rounds


def test_chain_through_a_dropped_row():
    """b ~ j1 ~ j2 with b !~ j2: j1 is dropped by the base and therefore drops nobody, j2 stays"""
    kept, rb, ri, rounds = run(2, [(0, 5)], [(0, 1)])
    assert kept == [False, True] and rb == [5, NONE] and ri == [NONE, 1] and rounds == 1


def test_dropped_by_the_base_and_by_an_earlier_kept_row():
    kept, rb, ri, _ = run(2, [(1, 3)], [(0, 1)])
    assert kept == [True, False]
    assert rb == [NONE, 3] and ri == [0, NONE], "the base's verdict names the representative: rep_base set, rep_incoming NONE"


def test_alternating_path_whose_first_row_has_a_base_partner():
    m = 9
    kept, rb, ri, rounds = run(m, [(0, 2), (0, 11)], [(i, i + 1) for i in range(m - 1)])
    assert kept == [i % 2 == 1 for i in range(m)], "the phase of the path flips: the odd rows stay"
    assert rb == [2] + [NONE] * (m - 1)
    assert ri == [NONE, 1, 1, 3, 3, 5, 5, 7, 7]
    assert rounds > 1
    # without the base partner the even rows stay
    kept, _, ri, _ = run(m, [], [(i, i + 1) for i in range(m - 1)])
    assert kept == [i % 2 == 0 for i in range(m)] and ri == [i - i % 2 for i in range(m)]


def test_lowest_kept_neighbour():
    """row 4 pairs with 1, 2 and 3; 1 is dropped by 0, so 2 is its lowest KEPT earlier neighbour -- until the base drops 2"""
    among = [(0, 1), (1, 4), (2, 4), (3, 4)]
    kept, rb, ri, _ = run(5, [], among)
    assert kept == [True, False, True, True, False] and ri == [0, 0, 2, 3, 2] and rb == [NONE] * 5
    kept, rb, ri, _ = run(5, [(2, 7)], among)
    assert kept == [True, False, False, True, False] and ri == [0, 0, NONE, 3, 3] and rb == [NONE, NONE, 7, NONE, NONE]


def test_without_a_list_among_the_batch_only_the_base_decides():
    kept, rb, ri, rounds = run(4, [(1, 9), (1, 4), (3, 0)], None)
    assert kept == [True, False, True, False] and rb == [NONE, 4, NONE, 0] and ri == [0, NONE, 2, NONE] and rounds == 0


def test_one_row():
    assert run(1, [], [])[:3] == ([True], [NONE], [0])
    assert run(1, [(0, 6)], [])[:3] == ([False], [6], [NONE])
    assert run(1, [(0, 6)], None)[:3] == ([False], [6], [NONE])
    assert run(1, [(0, 6)], None)[3] == 0 and run(1, [], [])[3] == 1


def test_cross_pairs_order_filter_and_threshold():
    class Orc:   # a score table in place of the oracle: row b against "query" j
        table = np.array([[95, 10, 95], [95, 95, 10], [10, 95, 96]], np.int64)   # [j][b]

        def score_all(self, base, q):
            return self.table[int(q[0])]
    base = np.zeros((3, 1), np.uint16)
    inc = np.arange(3, dtype=np.uint16).reshape(3, 1)
    lo, hi, sc = ref.cross_pairs(Orc(), base, inc, 95)
    assert list(zip(lo.tolist(), hi.tolist(), sc.tolist())) == [(0, 0, 95), (2, 0, 95), (0, 1, 95), (1, 1, 95), (1, 2, 95), (2, 2, 96)]
    lo, hi, _ = ref.cross_pairs(Orc(), base, inc, 96)
    assert (lo.tolist(), hi.tolist()) == ([2], [2]), "the threshold is inclusive"
    lo, hi, _ = ref.cross_pairs(Orc(), base, inc, 95, within=np.array([True, False]))   # shorter than the base: row 2 excluded too
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 0), (0, 1)]


def test_new_symbols_are_bound(mse):
    from mse import ffi
    vp, sz, u32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)
    want = {
        "mse_join_cross": (vp, [vp, vp, C.c_int64, vp, C.c_int, C.c_uint64]),
        "mse_pairs_kind": (C.c_int, [vp]),
        "mse_pairs_base_rows": (sz, [vp]),
        "mse_pairs_admit": (C.c_int, [vp, vp, C.POINTER(vp), u32p, u32p]),
        "mse_base_select": (vp, [vp, vp]),
    }
    for name, sig in want.items():
        assert ffi.SIGNATURES.get(name) == sig, name
        assert hasattr(C.CDLL(ffi.LIB_PATH), name), name
    assert hasattr(mse, "Admission") and hasattr(mse.Searcher, "near_duplicates_of") and hasattr(mse.VectorList, "select")
    assert hasattr(mse.RowPairs, "admit") and hasattr(mse.RowPairs, "kind") and hasattr(mse.RowPairs, "base_rows")
    assert hasattr(mse.DeviceGraph, "near_duplicates_of") and hasattr(mse.DeviceGraph, "insert_unique_rows")
    assert hasattr(mse.BuildGraph, "insert_unique_rows")
