"""Grouped graph search, the parts that need no device: the two statements of the rule (tests/grouped_graph_ref.py) agree on random
visited lists, the per-group statement is checked against a plain Python walk, and the new entry points refuse null handles."""
import ctypes as C

import numpy as np
import pytest

from grouped_graph_ref import cut, group_step, grouped_cut, ranked
from grouped_ref import GROUP_NONE, I64_MIN, ID_NONE

I64_MAX = np.iinfo(np.int64).max


def random_list(rng, n, g_len, n_groups, p_none, p_hole, score_kind):
    """One visited list: distinct ids, some of them at or past the grouping, holes in the middle, scores of the given kind."""
    ids = rng.choice(max(g_len + g_len // 3 + 8, 2 * n), n, replace=False).astype(np.uint32)
    if score_kind == "ties":
        sc = rng.integers(-2, 3, n).astype(np.int64)
    elif score_kind == "extremes":
        sc = rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1], np.int64), n)
    else:
        sc = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    hole = rng.random(n) < p_hole
    ids[hole], sc[hole] = ID_NONE, I64_MIN
    group_of = rng.integers(0, max(n_groups, 1), g_len).astype(np.uint32)
    group_of[rng.random(g_len) < p_none] = GROUP_NONE
    return ids, sc, group_of


def walk_step(ids, sc, n, group_of):
    """Statement 1 as a plain loop: the best record of every group by (score desc, id asc); the others become holes."""
    best = {}
    for i in range(min(n, len(ids))):
        r = int(ids[i])
        if r == ID_NONE or r >= len(group_of) or group_of[r] == GROUP_NONE:
            continue
        g = int(group_of[r])
        if g not in best or (-int(sc[i]), r) < (-int(sc[best[g]]), int(ids[best[g]])):
            best[g] = i
    out_i, out_s = ids.copy(), sc.copy()
    for i in range(min(n, len(ids))):
        r = int(ids[i])
        if r != ID_NONE and r < len(group_of) and group_of[r] != GROUP_NONE and best[int(group_of[r])] != i:
            out_i[i], out_s[i] = ID_NONE, I64_MIN
    return out_i, out_s


CASES = [(seed, kind) for seed in range(6) for kind in ("ties", "extremes", "wide")]


@pytest.mark.parametrize("seed,kind", CASES)
def test_the_two_statements_of_the_rule_agree(seed, kind):
    """Per group the best record (statement 1), then the sorted cut == the first record of every group in the ranked list (statement
    2), for every k: many equal scores, INT64_MIN / INT64_MAX scores, holes, ids past the grouping, lists cut short by n_visited."""
    rng = np.random.default_rng(1000 * seed + len(kind))
    n = int(rng.integers(1, 300))
    g_len = int(rng.integers(1, 400))
    ids, sc, group_of = random_list(rng, n, g_len, int(rng.integers(1, 40)), 0.25, 0.15, kind)
    n_vis = n if seed % 3 else int(rng.integers(0, n + 1))
    s_ids, s_sc = group_step(ids, sc, n_vis, group_of)
    # the per-group statement itself, against the plain loop
    w_ids, w_sc = walk_step(ids, sc, n_vis, group_of)
    assert np.array_equal(s_ids, w_ids) and np.array_equal(s_sc, w_sc)
    # entries at or past n_visited and ungrouped records are where they were
    assert np.array_equal(s_ids[n_vis:], ids[n_vis:]) and np.array_equal(s_sc[n_vis:], sc[n_vis:])
    gone = s_ids != ids
    assert np.all(s_ids[gone] == ID_NONE) and np.all(s_sc[gone] == I64_MIN) and np.array_equal(s_sc[~gone], sc[~gone])
    r_ids, r_sc = ranked(s_ids, s_sc, n_vis)
    for k in (1, 3, 10, n + 5):
        a = cut(r_ids, r_sc, k)
        b = grouped_cut(ids, sc, group_of, k, n_vis)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k


def test_all_none_and_one_group():
    rng = np.random.default_rng(5)
    ids, sc, _ = random_list(rng, 50, 200, 5, 0.0, 0.1, "ties")
    none = np.full(200, GROUP_NONE, np.uint32)
    a = group_step(ids, sc, 50, none)
    assert np.array_equal(a[0], ids) and np.array_equal(a[1], sc)
    one = np.full(300, 3, np.uint32)                     # covers every id: a single survivor, the lowest id among the best scores
    b = group_step(ids, sc, 50, one)
    live = np.flatnonzero(b[0] != ID_NONE)
    top = sc[ids != ID_NONE].max()
    assert live.size == 1 and b[0][live[0]] == ids[(sc == top) & (ids != ID_NONE)].min()


def test_grouped_graph_entry_points_refuse_null_handles(mse):
    from mse import ffi
    L = ffi.lib()
    assert L.mse_debug_visited_collapse(None, None, None, None, 8, None, 1) == -1 and "null searcher" in ffi.last_error()
    q16, q32 = np.zeros(128, np.uint16), np.zeros(128, np.float32)
    oi, os_ = np.full(4, 123, np.uint32), np.full(4, 456, np.int64)
    outs = (oi.ctypes.data_as(ffi.u32p), os_.ctypes.data_as(ffi.i64p), None, None, None)
    assert L.mse_disk_query_topk_grouped(None, None, None, None, None, None, 0, None, q16.ctypes.data_as(ffi.u16p), None, None, 1, 1, 4, 50, 4,
                                         *outs) == -1 and ffi.last_error()
    assert L.mse_disk_query_topk_grouped_f32(None, None, None, None, None, None, 0, None, q32.ctypes.data_as(ffi.f32p), None, 1, 1, 4, 50, 4,
                                             *outs) == -1 and ffi.last_error()
    t = C.c_void_p()
    assert L.mse_disk_query_submit_grouped_f32(None, None, None, None, None, None, 0, q32.ctypes.data_as(ffi.f32p), None, 1, 1, 4, 50, 4, *outs,
                                               None, None, C.byref(t)) == -1 and ffi.last_error() and not t.value
    assert np.all(oi == 123) and np.all(os_ == 456)
