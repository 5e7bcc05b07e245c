"""Grouped search, the parts that need no device: the numpy reference the GPU tests compare against is itself checked against a plain
Python walk; RowGroups refuses malformed arrays before any device work; and the new entry points fail loudly without a device."""
import ctypes as C

import numpy as np
import pytest

from grouped_ref import GROUP_NONE, I64_MIN, ID_NONE, collapse_positions, grouped_topk


def walk(ranked_ids, group_of):
    """The reference's loop (src/main.rs:902-917): keep an entry unless its group was seen."""
    seen, keep = set(), []
    for pos, r in enumerate(ranked_ids):
        g = group_of[r] if r < len(group_of) else GROUP_NONE
        if g == GROUP_NONE:
            keep.append(pos)
        elif g not in seen:
            seen.add(g)
            keep.append(pos)
    return keep


@pytest.mark.parametrize("seed", range(8))
def test_collapse_reference_equals_the_walk(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    g_len = int(rng.integers(0, n + 1))          # a grouping shorter than the rows
    group_of = rng.integers(0, max(g_len, 1), g_len).astype(np.uint32)
    group_of[rng.random(g_len) < 0.3] = GROUP_NONE
    ranked = rng.permutation(n)[:int(rng.integers(1, n + 1))]
    assert list(collapse_positions(ranked, group_of)) == walk(list(ranked), list(group_of))


@pytest.mark.parametrize("seed", range(6))
def test_grouped_topk_reference_equals_sort_and_walk(seed):
    rng = np.random.default_rng(100 + seed)
    n, k = 40, 7
    scores = rng.integers(-3, 4, n).astype(np.int64)       # many ties
    scores[rng.integers(0, n)] = I64_MIN
    scores[rng.integers(0, n)] = np.iinfo(np.int64).max
    group_of = rng.integers(0, 6, n).astype(np.uint32)
    group_of[rng.random(n) < 0.2] = GROUP_NONE
    allowed = rng.random(n) < 0.6 if seed % 2 else None
    rows = [i for i in range(n) if allowed is None or allowed[i]]
    ranked = sorted(rows, key=lambda i: (-int(scores[i]), i))
    keep = [ranked[p] for p in walk(ranked, list(group_of))][:k]
    ws, wi = grouped_topk(scores, group_of, k, allowed)
    assert list(wi[:len(keep)]) == keep and (wi[len(keep):] == ID_NONE).all()
    assert list(ws[:len(keep)]) == [int(scores[i]) for i in keep] and (ws[len(keep):] == I64_MIN).all()


def test_row_groups_argument_checks(mse):
    with pytest.raises(TypeError):
        mse.RowGroups(np.zeros(4, np.float32))
    with pytest.raises(TypeError):
        mse.RowGroups(np.zeros(4, bool))
    with pytest.raises(ValueError):
        mse.RowGroups(np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError):
        mse.RowGroups(np.array([0, -2], np.int64))
    with pytest.raises(ValueError):
        mse.RowGroups(np.array([0, 1 << 32], np.int64))
    assert mse.GROUP_NONE == GROUP_NONE


def test_grouped_entry_points_fail_loudly_without_a_device(mse):
    from mse import ffi
    L = ffi.lib()
    if L.mse_device_count() > 0:
        pytest.skip("a device is present")
    g = np.zeros(4, np.uint32)
    assert not L.mse_groups_from_host(g.ctypes.data_as(ffi.u32p), 4)
    assert ffi.last_error()
    with pytest.raises(mse.MseError):
        mse.RowGroups(g)
    with pytest.raises(mse.MseError):
        mse.RowGroups.from_device(None, 4)
    # null handles: an error with the message set, nothing dereferenced
    out = (C.c_uint32 * 3)()
    assert L.mse_searcher_grouped_stats(None, out) == -1 and ffi.last_error()
    assert L.mse_bruteforce_topk_grouped_f16(None, None, None, None, 1, 1, 0, None, None) == -1 and "null searcher" in ffi.last_error()
    assert L.mse_bruteforce_topk_grouped_f16_dev(None, None, None, None, 1, 1, 0, 0, None, None) == -1 and "null searcher" in ffi.last_error()
    assert L.mse_index_search_grouped(None, None, None, None, 1, 1, None, None) == -1 and "null index" in ffi.last_error()
    assert L.mse_debug_collapse_topk(None, None, None, 1, 1, 1, None, None) == -1 and "null searcher" in ffi.last_error()
    assert L.mse_groups_len(None) == 0 and L.mse_groups_count(None) == 0
    L.mse_groups_free(None)
