"""Host-side argument checks of mse.RowFilter (no device needed)."""
import numpy as np
import pytest


def test_row_filter_argument_checks(mse):
    with pytest.raises(ValueError):
        mse.RowFilter(np.array([1, 2, 3]))                 # ids without n_rows
    with pytest.raises(ValueError):
        mse.RowFilter(np.array([1, -2]), n_rows=10)        # not a row id
    with pytest.raises(ValueError):
        mse.RowFilter(np.ones(3, bool), n_rows=4)          # a mask has one entry per row
    with pytest.raises(TypeError):
        mse.RowFilter(np.array([0.5]))


def test_filter_entry_points_are_bound(mse):
    from mse import ffi
    for name in ("mse_filter_from_bits", "mse_filter_from_ids", "mse_filter_free", "mse_filter_len", "mse_filter_count",
                 "mse_bruteforce_topk_filtered_f16", "mse_bruteforce_topk_filtered_f16_dev", "mse_dispatcher_topk_filtered_f16",
                 "mse_index_search_filtered"):
        assert name in ffi.SIGNATURES
