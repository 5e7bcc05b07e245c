"""Filtered graph search, the part that needs no device: mse_filtered_plan -- what MSE_FILTERED_AUTO will do -- is a pure host
function of (graph rows, allowed rows, search_list, de-duplication on?), and the new entry points are declared, exported and bound."""
import re
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ceil_div(a, b):
    return -(-a // b)


# (n, allowed, L, dedup) -> (regime, effective search_list); the rule of include/mse.h / DESIGN 3.9, restated by hand
PLAN_TABLE = [
    ((10_000_000, 0, 200, False), ("list", 200)),               # nothing allowed: all padding, no launch
    ((10_000_000, 0, 200, True), ("list", 200)),
    ((10_000_000, 10_000_000, 200, False), ("graph", 200)),      # everything allowed: the unfiltered search
    ((10_000_000, 10_000_000, 1024, True), ("graph", 1024)),
    ((10_000_000, 5_000_000, 200, False), ("graph", 400)),
    ((10_000_000, 1_953_125, 200, False), ("graph", 1024)),      # the last allowed count with L' <= 1024 ...
    ((10_000_000, 1_953_124, 200, False), ("list", 200)),        # ... and the first with L' = 1025
    ((10_000_000, 1_953_124, 200, True), ("graph", 1024)),       # de-duplication on: the longest search instead of the scan
    ((10_000_000, 1, 1, False), ("list", 1)),
    ((20_000, 3_907, 200, False), ("graph", 1024)),
    ((20_000, 3_906, 200, False), ("list", 200)),
    ((20_000, 19_999, 12, False), ("graph", 13)),                # ceil(12 * 20000 / 19999) = 13
    ((1, 1, 1024, False), ("graph", 1024)),
    ((4_294_967_295, 4_194_304, 1, False), ("graph", 1024)),     # ceil(2^32 - 1 / 2^22) = 1024: no overflow on the way
    ((4_294_967_295, 4_194_303, 1, False), ("list", 1)),
]


@pytest.mark.parametrize("args,want", PLAN_TABLE)
def test_filtered_plan_table(args, want):
    import mse
    n, allowed, L, dedup = args
    if allowed:                                                   # the table agrees with the rule as the issue states it
        widened = ceil_div(L * n, allowed)
        rule = ("graph", max(L, widened)) if widened <= 1024 else (("graph", 1024) if dedup else ("list", L))
        assert rule == want
    assert mse.filtered_plan(n, allowed, L, dedup) == want


def test_filtered_plan_boundary_sweep():
    """For every search_list the boundary sits where ceil(L n / c) crosses 1024 -- checked on both sides."""
    import mse
    n = 10_000_000
    for L in (1, 12, 100, 200, 999, 1024):
        c_last = ceil_div(L * n, 1024)                           # smallest c with L n / c <= 1024
        assert ceil_div(L * n, c_last) <= 1024
        assert mse.filtered_plan(n, c_last, L) == ("graph", max(L, ceil_div(L * n, c_last)))
        if c_last > 1:
            assert ceil_div(L * n, c_last - 1) > 1024
            assert mse.filtered_plan(n, c_last - 1, L) == ("list", L)
            assert mse.filtered_plan(n, c_last - 1, L, True) == ("graph", 1024)


@pytest.mark.parametrize("L", [0, 1025, 5000])
def test_filtered_plan_refuses_a_search_list_out_of_range(L):
    import mse
    with pytest.raises(mse.MseError, match="search_list"):
        mse.filtered_plan(1000, 10, L)


def test_filtered_plan_argument_errors_write_nothing():
    import ctypes as C
    import mse
    from mse import ffi
    rg, eff = C.c_int(77), C.c_size_t(88)
    assert ffi.lib().mse_filtered_plan(1000, 1001, 10, 0, C.byref(rg), C.byref(eff)) != 0      # more allowed rows than rows
    assert "allowed" in ffi.last_error() and (rg.value, eff.value) == (77, 88)
    assert ffi.lib().mse_filtered_plan(1000, 10, 0, 0, C.byref(rg), C.byref(eff)) != 0
    assert (rg.value, eff.value) == (77, 88)
    assert ffi.lib().mse_filtered_plan(1000, 10, 10, 0, None, C.byref(eff)) != 0
    assert ffi.lib().mse_filtered_plan(1000, 10, 10, 0, C.byref(rg), None) != 0
    from mse import diskann
    with pytest.raises(ValueError):
        diskann._regime("fastest")                                                                  # a regime is one of auto / graph / list
    assert [diskann._regime(r) for r in ("auto", "graph", "list")] == [0, 1, 2]


NEW_SYMBOLS = ["mse_filtered_plan", "mse_disk_search_batch_filtered", "mse_disk_query_topk_filtered", "mse_disk_query_topk_filtered_f32",
               "mse_disk_query_submit_filtered_f32"]


def test_new_entry_points_are_declared_exported_and_bound():
    import ctypes as C
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES, name
        assert getattr(ffi.lib(), name) is not None, name
    for name, val in (("MSE_FILTERED_AUTO", 0), ("MSE_FILTERED_GRAPH", 1), ("MSE_FILTERED_LIST", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), text), name
    # every filtered call takes the arguments of the call it extends, plus the filter (and the regime)
    sig = ffi.SIGNATURES
    assert len(sig["mse_disk_search_batch_filtered"][1]) == len(sig["mse_disk_search_batch"][1]) + 1
    assert len(sig["mse_disk_query_topk_filtered"][1]) == len(sig["mse_disk_query_topk"][1]) + 2
    assert len(sig["mse_disk_query_topk_filtered_f32"][1]) == len(sig["mse_disk_query_topk_f32"][1]) + 2
    assert len(sig["mse_disk_query_submit_filtered_f32"][1]) == len(sig["mse_disk_query_submit_f32"][1]) + 2
    assert sig["mse_filtered_plan"][0] is C.c_int
