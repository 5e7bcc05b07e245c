"""Host-side checks of the filter algebra's surface (no device needed)."""
import ctypes as C

import pytest

NAMES = ("mse_filter_combine", "mse_filter_not", "mse_filter_from_descriptors", "mse_filter_from_scores", "mse_filter_from_bits_dev",
         "mse_filter_to_bits", "mse_filter_read_ids")


def test_filter_ops_are_bound(mse):
    from mse import ffi
    for name in NAMES:
        assert name in ffi.SIGNATURES, name
        assert getattr(ffi.lib(), name) is not None
    for name in NAMES[:5]:
        assert ffi.SIGNATURES[name][0] is C.c_void_p, name                  # creators return a handle
    for name in NAMES[5:]:
        assert ffi.SIGNATURES[name][0] is C.c_int, name
    assert ffi.SIGNATURES["mse_filter_from_scores"][1][2] is C.c_int64       # the threshold is a full i64 score


def test_a_foreign_operand_is_a_type_error(mse):
    f = mse.RowFilter.from_handle(None)
    for op in (lambda: f & 3, lambda: f | 3, lambda: f ^ 3, lambda: f - 3, lambda: 3 & f, lambda: f & [True]):
        with pytest.raises(TypeError):
            op()


def test_descriptor_ranges_are_checked_before_any_call(mse):
    class FakeCodes:
        n_desc, _h = 4, None
    for bad in ({4: (0, 1)}, {-1: (0, 1)}, {0: (0, 256)}, {1: (-1, 3)}):
        with pytest.raises(ValueError):
            mse.RowFilter.from_descriptors(FakeCodes(), bad)
