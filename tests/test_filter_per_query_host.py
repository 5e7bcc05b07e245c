"""A filter per query (include/mse.h "a filter per query"), the part that needs no device: the three entry points are declared, exported
and bound with the arguments of their single-filter twins; a null filters array and an unknown regime are refused before anything else
is looked at; the Python layer tells a sequence of filters from one filter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mse_disk_query_topk_filtered_each", "mse_disk_query_topk_filtered_each_f32", "mse_disk_search_batch_filtered_each"]


def declaration(text, name):
    """the argument list of `name` as include/mse.h declares it, one string per argument"""
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_exported_and_bound():
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    sig = ffi.SIGNATURES
    for name in NEW_SYMBOLS:
        assert name in sig and sig[name][0] is C.c_int, name
        assert getattr(ffi.lib(), name) is not None, name
        assert len(declaration(text, name)) == len(sig[name][1]), name
    # each twin takes its single-filter call's arguments with the array where the filter stands (the top-k forms: plus the grouping)
    for each, twin, extra in (("mse_disk_query_topk_filtered_each", "mse_disk_query_topk_filtered", 1),
                              ("mse_disk_query_topk_filtered_each_f32", "mse_disk_query_topk_filtered_f32", 1),
                              ("mse_disk_search_batch_filtered_each", "mse_disk_search_batch_filtered", 0)):
        d_each, d_twin = declaration(text, each), declaration(text, twin)
        assert len(d_each) == len(d_twin) + extra
        assert d_each[4] == "const mse_filter* const* filters" and d_twin[4] == "const mse_filter* f"
        assert sig[each][1][4] is not sig[twin][1][4] and sig[each][1][4]._type_ is C.c_void_p      # a pointer to handles, not a handle
        if extra:
            assert d_each[6] == "const mse_groups* groups"
            assert [a.split()[-1] for a in d_each[:6] + d_each[7:]] == ["filters" if a.endswith(" f") else a.split()[-1] for a in d_twin]
            assert sig[each][1][:4] + sig[each][1][5:6] + sig[each][1][7:] == sig[twin][1][:4] + sig[twin][1][5:]
        else:
            assert sig[each][1][:4] + sig[each][1][5:] == sig[twin][1][:4] + sig[twin][1][5:]
    # the counter of what shared a launch: declared, bound, and a null graph is refused
    assert len(declaration(text, "mse_graph_coalescer_groups")) == len(sig["mse_graph_coalescer_groups"][1]) == 2
    out = (C.c_uint64 * 2)(7, 7)
    assert ffi.lib().mse_graph_coalescer_groups(None, out) != 0 and list(out) == [7, 7]
    # the header no longer promises the old sharing rule
    assert "only with requests of the same filter object, regime and effective search_list" not in text


def outputs(nq=3, k=4):
    oi, os_, cnt = np.full((nq, k), 123, np.uint32), np.full((nq, k), 456, np.int64), np.full((3, nq), 789, np.uint32)
    u32, i64 = C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    ptrs = (oi.ctypes.data_as(u32), os_.ctypes.data_as(i64), cnt[0].ctypes.data_as(u32), cnt[1].ctypes.data_as(u32), cnt[2].ctypes.data_as(u32))
    return (oi, os_, cnt), ptrs


def untouched(arrays):
    oi, os_, cnt = arrays
    return bool(np.all(oi == 123) and np.all(os_ == 456) and np.all(cnt == 789))


def test_null_array_and_unknown_regime_are_refused_first():
    """Both are found before the handles are looked at, so no device is needed to see them: non-zero, the message, nothing written."""
    from mse import ffi
    lib = ffi.lib()
    nq, k = 3, 4
    q16, q32 = np.zeros((nq, 64), np.uint16), np.zeros((nq, 64), np.float32)
    u16, f32 = C.POINTER(C.c_uint16), C.POINTER(C.c_float)
    no_filters = (C.c_void_p * nq)(None, None, None)
    for filters, regime, word in ((None, 1, "null filters array"), (None, 0, "null filters array"), (no_filters, 7, "unknown regime"),
                                  (no_filters, -1, "unknown regime")):
        arrays, outs = outputs(nq, k)
        assert lib.mse_disk_query_topk_filtered_each(None, None, None, None, filters, regime, None, None, q16.ctypes.data_as(u16), None, None,
                                                     nq, 1, 4, 50, k, *outs) != 0
        assert word in ffi.last_error() and untouched(arrays)
        assert lib.mse_disk_query_topk_filtered_each_f32(None, None, None, None, filters, regime, None, None, q32.ctypes.data_as(f32), None,
                                                         nq, 1, 4, 50, k, *outs) != 0
        assert word in ffi.last_error() and untouched(arrays)
    arrays, outs = outputs(nq, 50)
    bl = np.full(nq, 789, np.uint32)
    assert lib.mse_disk_search_batch_filtered_each(None, None, None, None, None, None, q16.ctypes.data_as(u16), None, None, nq, 1, 4, 50, outs[0],
                                                   outs[1], bl.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, 0, *outs[2:]) != 0
    assert "null filters array" in ffi.last_error() and untouched(arrays) and np.all(bl == 789)
    # a valid array over null handles is the next thing found, in the words of the single-filter call
    arrays, outs = outputs(nq, k)
    assert lib.mse_disk_query_topk_filtered_each(None, None, None, None, no_filters, 1, None, None, q16.ctypes.data_as(u16), None, None, nq, 1, 4,
                                                 50, k, *outs) != 0
    assert "null" in ffi.last_error() and untouched(arrays)


def test_python_tells_a_sequence_from_one_filter():
    from mse import diskann
    assert diskann._filter_array(None, 3) is None
    arr = diskann._filter_array([None, None, None], 3)
    assert len(arr) == 3 and all(h is None for h in arr)
    with pytest.raises(diskann.MseError, match="2 filters for 3 queries"):
        diskann._filter_array([None, None], 3)
    with pytest.raises(TypeError):
        diskann._filter_array([None, "half", None], 3)
    assert diskann.QueryTickets.submit.__defaults__[-1] is diskann._OWN_FILTER
