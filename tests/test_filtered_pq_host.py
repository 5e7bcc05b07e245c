"""Host side of the filtered PQ flat scan: the plan function (pure host), and that every new entry point is declared, exported and bound."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_INT = ["mse_pq_scan_topk_filtered", "mse_pq_scan_topk_batch_filtered", "mse_pq_scan_topk_block_filtered", "mse_pq_filtered_plan",
           "mse_debug_pq_group_max_filtered", "mse_debug_pq4_group_max_filtered"]
SCAN, LIST = 1, 2


def plan(n, allowed, nq):
    from mse import ffi
    m = C.c_int(-1)
    rc = ffi.lib().mse_pq_filtered_plan(n, allowed, nq, C.byref(m))
    return rc, m.value


def test_entry_points_are_declared_exported_and_bound(mse):
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_INT:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES and ffi.SIGNATURES[name][0] is C.c_int, name
        assert getattr(ffi.lib(), name) is not None, name
    assert re.search(r"\bmse_filter\s*\*\s*mse_graph_live_filter\s*\(", text)
    assert ffi.SIGNATURES["mse_graph_live_filter"] == (C.c_void_p, [C.c_void_p, C.c_int]) and ffi.lib().mse_graph_live_filter is not None
    for macro, value in (("MSE_PQ_FILTER_AUTO", 0), ("MSE_PQ_FILTER_SCAN", 1), ("MSE_PQ_FILTER_LIST", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    assert mse.vector.PQ_FILTER_MODES == {"auto": 0, "scan": 1, "list": 2}
    # the argument lists follow the unfiltered calls, with the filter after the codes and the mode before the outputs
    for name, base in (("mse_pq_scan_topk_filtered", "mse_pq_scan_topk"), ("mse_pq_scan_topk_batch_filtered", "mse_pq_scan_topk_batch"),
                       ("mse_pq_scan_topk_block_filtered", "mse_pq_scan_topk_block")):
        a, b = ffi.SIGNATURES[name][1], ffi.SIGNATURES[base][1]
        assert len(a) == len(b) + 2 and a[:2] == b[:2] and a[2] is C.c_void_p and a[3:3 + len(b) - 2 - 2] == b[2:len(b) - 2], name
    for cls in (mse.DeviceGraph, mse.BuildGraph):
        assert callable(cls.live_filter)
    for meth in ("scan_topk_filtered", "scan_topk_batch_filtered", "filtered_plan", "debug_group_max_filtered", "debug_group_max4_filtered"):
        assert callable(getattr(mse.ProductQuantizer, meth)), meth


def test_entry_points_fail_loudly_without_their_objects(mse):
    from mse import ffi
    L = ffi.lib()
    sc = (C.c_int64 * 4)(7, 7, 7, 7)
    ids = (C.c_uint32 * 4)(9, 9, 9, 9)
    q = (C.c_float * 1152)()
    assert L.mse_pq_scan_topk_filtered(None, None, None, None, q, None, 10, 4, 0, sc, ids) != 0
    assert "null" in ffi.last_error() and list(sc) == [7] * 4 and list(ids) == [9] * 4
    assert L.mse_pq_scan_topk_batch_filtered(None, None, None, None, q, 1, None, 10, 4, 0, sc, ids) != 0
    assert "null" in ffi.last_error() and list(sc) == [7] * 4 and list(ids) == [9] * 4
    assert L.mse_pq_scan_topk_block_filtered(None, None, None, None, q, 1, None, 10, 4, 0, 0, sc) != 0
    assert "null" in ffi.last_error() and list(sc) == [7] * 4
    assert not L.mse_graph_live_filter(None, 0) and "graph_live_filter" in ffi.last_error()
    with pytest.raises(ffi.MseError, match="closed"):
        g = mse.DeviceGraph.__new__(mse.DeviceGraph)
        g._h = None
        g.live_filter()


@pytest.mark.parametrize("n", [1, 64, 4097, 10_000_000, 3_000_000_000])
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 2048])
def test_plan_is_monotone(mse, n, nq):
    """Once LIST is chosen, fewer allowed rows never flip it back to SCAN; allowed = 0 is LIST; the answer is one of the two modes."""
    assert plan(n, 0, nq) == (0, LIST)
    counts = sorted({0, 1, 2, n // 4096, n // 257, n // 64, n // 16, n // 9, n // 8, n // 4, n // 3, n // 2, n // 2 + 1, n - 1, n})
    counts = [a for a in counts if 0 <= a <= n]
    answers = []
    for a in counts:
        rc, m = plan(n, a, nq)
        assert rc == 0 and m in (SCAN, LIST), (a, rc, m)
        answers.append(m)
    seen_scan = False
    for m in answers:                                        # ascending allowed: LIST ... LIST SCAN ... SCAN
        seen_scan = seen_scan or m == SCAN
        assert not (seen_scan and m == LIST), (counts, answers)
    assert mse.ProductQuantizer.filtered_plan(n, 0, nq) == "list"


def test_plan_errors(mse):
    from mse import ffi
    rc, m = plan(100, 101, 1)
    assert rc != 0 and m == -1 and "more allowed rows than codes" in ffi.last_error()
    rc, m = plan(100, 50, 0)
    assert rc != 0 and m == -1 and "nq" in ffi.last_error()
    assert ffi.lib().mse_pq_filtered_plan(100, 50, 1, None) != 0 and "null" in ffi.last_error()
    with pytest.raises(ffi.MseError):
        mse.ProductQuantizer.filtered_plan(10, 11, 1)
