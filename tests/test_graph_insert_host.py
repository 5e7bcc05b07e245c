"""Insert rows into freed slots (include/mse.h), the part that needs no device: the Python wrapper's argument checks on both graph
classes, and the three new entry points declared, exported, bound and failing loudly when there is nothing to run on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_graph_delete_host import fake_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 1152
NEW_SYMBOLS = ["mse_graph_insert_rows", "mse_graph_insert_rows_dev", "mse_debug_base_norm_bits"]


class FakeVecs:
    _h = 1
    d_emb = D


class FakeSearcher:
    _h = 1
    vecs = FakeVecs()


def open_graph(mse, name):
    """a graph object whose handle is set: the argument checks that come after the closed-graph check are reached, and every one of
    them raises before the library is called (the handle is never used)"""
    g = fake_graph(mse, getattr(mse, name))
    g._h = 1
    return g


@pytest.mark.parametrize("cls", ["DeviceGraph", "BuildGraph"])
def test_insert_rows_argument_checks(mse, cls):
    g = fake_graph(mse, getattr(mse, cls))
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    rows = np.zeros((2, D), np.uint16)
    with pytest.raises(TypeError, match="IndexBuildConfig"):
        g.insert_rows(FakeSearcher(), [1, 2], rows, {"r": 32}, 0)
    for bad in (-1, 1.5, True, "8"):
        with pytest.raises(ValueError, match="batch"):
            g.insert_rows(FakeSearcher(), [1, 2], rows, cfg, 0, batch=bad)
    with pytest.raises(mse.MseError, match="searcher"):
        g.insert_rows(None, [1, 2], rows, cfg, 0)
    for bad in (-1, 1 << 32, 0.5, True, None):
        with pytest.raises(ValueError, match="start"):
            g.insert_rows(FakeSearcher(), [1, 2], rows, cfg, bad)
    with pytest.raises(mse.MseError, match="closed"):                      # a closed graph is refused before anything is read
        g.insert_rows(FakeSearcher(), [1, 2], rows, cfg, 0)
    g = open_graph(mse, cls)
    try:
        with pytest.raises(TypeError, match="slots"):
            g.insert_rows(FakeSearcher(), [0.5, 2], rows, cfg, 0)
        with pytest.raises(ValueError, match="slots"):
            g.insert_rows(FakeSearcher(), [-1, 2], rows, cfg, 0)

        class NoRows:
            _h = 1
        with pytest.raises(mse.MseError, match="searcher"):                # the width of a row comes from the searcher's rows
            g.insert_rows(NoRows(), [1, 2], rows, cfg, 0)
        with pytest.raises(ValueError, match="one row"):                   # a short array never reaches the library
            g.insert_rows(FakeSearcher(), [1, 2, 3], rows, cfg, 0)
        with pytest.raises(ValueError, match="one row"):
            g.insert_rows(FakeSearcher(), [1, 2], rows[:, :D - 32], cfg, 0)
        with pytest.raises(TypeError, match="f16"):
            g.insert_rows(FakeSearcher(), [1, 2], rows.astype(np.float32), cfg, 0)
        with pytest.raises(ValueError, match="descriptors"):
            g.insert_rows(FakeSearcher(), [1, 2], rows, cfg, 0, descriptors=np.zeros(3, np.uint8))
        with pytest.raises(ValueError, match="has_url"):
            g.insert_rows(FakeSearcher(), [1, 2], rows, cfg, 0, has_url=[1, 1, 1])

        class DeviceRows:                                                  # stands for a tensor: data_ptr() selects the _dev entry
            def __init__(self, numel, size=2, contiguous=True, cuda=True):
                self._n, self._s, self._c, self.is_cuda = numel, size, contiguous, cuda

            def data_ptr(self):
                return 4096

            def numel(self):
                return self._n

            def element_size(self):
                return self._s

            def is_contiguous(self):
                return self._c
        with pytest.raises(ValueError, match="one row"):
            g.insert_rows(FakeSearcher(), [1, 2], DeviceRows(D), cfg, 0)
        with pytest.raises(TypeError, match="2-byte"):
            g.insert_rows(FakeSearcher(), [1, 2], DeviceRows(2 * D, size=4), cfg, 0)
        with pytest.raises(ValueError, match="contiguous"):
            g.insert_rows(FakeSearcher(), [1, 2], DeviceRows(2 * D, contiguous=False), cfg, 0)
        with pytest.raises(TypeError, match="device"):
            g.insert_rows(FakeSearcher(), [1, 2], DeviceRows(2 * D, cuda=False), cfg, 0)
    finally:
        g._h = None                                                        # (never a real handle: nothing to free)
    assert mse.INSERT_STATS == ("inserted", "batches")


def test_insert_entry_points_are_declared_exported_and_bound():
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES and ffi.SIGNATURES[name][0] is C.c_int, name
        assert getattr(ffi.lib(), name) is not None, name
    assert len(ffi.SIGNATURES["mse_graph_insert_rows"][1]) == 13 and len(ffi.SIGNATURES["mse_graph_insert_rows_dev"][1]) == 13
    for phrase in ("insert rows into freed slots", "never lowered", "must be writable", "wholly before or wholly after"):
        assert phrase in text, phrase                                      # the contract is written where the delete's is


def test_insert_entry_points_fail_loudly_without_their_objects(mse):
    from mse import ffi
    L = ffi.lib()
    stats = (C.c_uint64 * 2)(7, 7)
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    slots = (C.c_uint32 * 1)(3)
    row = (C.c_uint16 * D)()
    assert L.mse_graph_insert_rows(None, None, None, None, slots, 1, row, None, None, 0, C.byref(cfg), 0, stats) != 0
    assert "graph_insert_rows" in ffi.last_error() and "null" in ffi.last_error() and list(stats) == [7, 7]
    assert L.mse_graph_insert_rows_dev(None, None, None, None, slots, 1, None, None, None, 0, C.byref(cfg), 0, stats) != 0
    assert "graph_insert_rows_dev" in ffi.last_error() and list(stats) == [7, 7]
    bits = (C.c_uint32 * 3)(9, 9, 9)
    assert L.mse_debug_base_norm_bits(None, bits) != 0 and "debug_base_norm_bits" in ffi.last_error() and list(bits) == [9, 9, 9]
