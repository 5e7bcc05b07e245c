"""Row filters across shards (include/mse.h mse_filter_slice / mse_filter_concat / mse_shard_filter), the part that needs no device: the
word rules of the two kernels restated in numpy on packbits(..., bitorder="little") masks and checked against plain boolean slicing, the
group's split rule, the per-shard resolution of the two AUTO plans (both pure host functions), and the new entry points declared,
exported and bound."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_WORDS = 8          # a filter's bitmap is whole 256-row tiles: 8 words


def to_words(mask):
    """a boolean mask as the filter's bitmap: LSB-first u32 words padded with zero words to whole tiles"""
    n_words = -(-len(mask) // 256) * TILE_WORDS
    b = np.zeros(max(n_words, 1) * 4, np.uint8)
    p = np.packbits(np.asarray(mask, bool), bitorder="little")
    b[:p.size] = p
    return b.view("<u4")[:n_words].copy()


def to_mask(words, n_rows):
    return np.unpackbits(words.view(np.uint8), count=n_rows, bitorder="little").astype(bool)


def row_mask(w, n_rows):
    r0 = w * 32
    if r0 >= n_rows:
        return 0
    return 0xFFFFFFFF >> (32 - (n_rows - r0)) if r0 + 32 > n_rows else 0xFFFFFFFF


def slice_words(src, src_rows, first_row, n_rows):
    """slice_words_kernel: out[w] = funnel(in[w0 + w], in[w0 + w + 1]) >> (first_row & 31), masked to n_rows; the source reads as zero
    at and past its words and its rows"""
    n_words = -(-n_rows // 256) * TILE_WORDS
    out = np.zeros(n_words, "<u4")
    w0, sh = first_row >> 5, first_row & 31

    def rd(s):
        return (int(src[s]) & row_mask(s, src_rows)) if s < len(src) else 0
    for w in range(n_words):
        out[w] = (((rd(w0 + w + 1) << 32) | rd(w0 + w)) >> sh) & 0xFFFFFFFF & row_mask(w, n_rows)
    return out


def place_words(out, n_rows, part, part_rows, first_row):
    """place_words_kernel: thread j owns destination word (first_row >> 5) + j = funnel(part[j - 1], part[j]) >> (32 - (first_row & 31))"""
    pw = -(-part_rows // 32)
    w0, sh = first_row >> 5, first_row & 31

    def rd(j):
        return (int(part[j]) & row_mask(j, part_rows)) if 0 <= j < pw else 0
    for j in range(pw + 1):
        v = (((rd(j) << 32) | rd(j - 1)) >> (32 - sh)) & 0xFFFFFFFF & row_mask(w0 + j, n_rows)
        if v:
            out[w0 + j] |= v


def shard_range(n, g, G):
    base, rem = divmod(n, G)
    lo = g * base + min(g, rem)
    return lo, lo + base + (1 if g < rem else 0)


@pytest.mark.parametrize("shift", [0, 1, 31])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 255, 256, 257, 700])
def test_slice_rule_equals_boolean_slicing(shift, n_rows):
    rng = np.random.default_rng(n_rows * 32 + shift)
    n = 1500
    for m in (np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.5):
        src = to_words(m)
        for first in (shift, 320 + shift, n - n_rows // 2 - 32 + shift, n + 64 + shift):     # inside, reaching past the end, wholly past it
            want = np.zeros(n_rows, bool)
            got_rows = m[first:first + n_rows]
            want[:len(got_rows)] = got_rows
            out = slice_words(src, n, first, n_rows)
            assert np.array_equal(to_mask(out, n_rows), want), (first, n_rows)
            assert np.array_equal(out, to_words(want)), "tail word and tile padding are zero"


def test_slice_ignores_source_bits_past_the_source_length():
    src = np.full(8, 0xFFFFFFFF, "<u4")                 # a bitmap that breaks the invariant: bits set past its 40 rows
    out = slice_words(src, 40, 33, 64)
    assert to_mask(out, 64).tolist() == [True] * 7 + [False] * 57


@pytest.mark.parametrize("n,G", [(2999, 4), (2999, 3), (2999, 1), (5, 8), (8193, 7), (64, 4)])
def test_concat_of_the_groups_slices_is_the_filter(n, G):
    """the split rule: contiguous, the remainder on the first shards -- 2 999 rows over 4 shards start at 750, 1 500 and 2 250"""
    rng = np.random.default_rng(n + G)
    m = rng.random(n) < 0.5
    m[[0, n - 1]] = True
    src = to_words(m)
    bounds = [shard_range(n, g, G) for g in range(G)]
    assert bounds[0][0] == 0 and bounds[-1][1] == n and all(bounds[g][1] == bounds[g + 1][0] for g in range(G - 1))
    sizes = [hi - lo for lo, hi in bounds]
    assert sizes == sorted(sizes, reverse=True) and max(sizes) - min(sizes) <= 1 and sizes.count(max(sizes)) in (n % G, G)
    if (n, G) == (2999, 4):
        assert [lo for lo, _ in bounds] == [0, 750, 1500, 2250]
    out = np.zeros_like(src)
    for lo, hi in bounds:
        if hi > lo:
            part = slice_words(src, n, lo, hi - lo)
            assert np.array_equal(to_mask(part, hi - lo), m[lo:hi])
            place_words(out, n, part, hi - lo, lo)
    assert np.array_equal(out, src)


def test_concat_rule_with_a_gap_and_a_shared_boundary_word():
    rng = np.random.default_rng(5)
    a, b, c = rng.random(45) < 0.5, np.ones(30, bool), rng.random(100) < 0.5
    n = 300
    want = np.zeros(n, bool)
    want[3:48], want[48:78], want[130:230] = a, b, c            # a and b share word 1; rows 78 .. 129 are a gap
    out = to_words(np.zeros(n, bool))
    for part, first in ((c, 130), (a, 3), (b, 48)):              # any order
        place_words(out, n, to_words(part), len(part), first)
    assert np.array_equal(out, to_words(want))


def test_auto_plans_resolve_per_shard():
    """Under AUTO every shard asks the plan with ITS rows and ITS count, so one call may run different regimes on different shards;
    both plans are pure host functions of those numbers."""
    import ctypes as C
    import mse
    from mse import ffi
    n, G, L = 4_000_000, 4, 200
    bounds = [shard_range(n, g, G) for g in range(G)]
    counts = [1_000_000, 195_313, 195_312, 0]                    # all allowed | last count with L' <= 1024 | first with 1025 | none
    want = [("graph", 200), ("graph", 1024), ("list", 200), ("list", 200)]
    got = [mse.filtered_plan(hi - lo, c, L) for (lo, hi), c in zip(bounds, counts)]
    assert got == want
    assert mse.filtered_plan(n, sum(counts), L) == ("graph", 576)    # the whole index would have planned something else again

    def pq_plan(n_codes, allowed, nq):
        m = C.c_int(-1)
        ffi.check(ffi.lib().mse_pq_filtered_plan(n_codes, allowed, nq, C.byref(m)), "mse_pq_filtered_plan")
        return m.value
    SCAN, LIST = 1, 2
    # the rule of csrc/api_pq.hip by hand: list cost nq (allowed x 68 x 2 + 1.2e6 x 68) against passes x n x 68
    n_sh = 25_000_000
    for allowed, nq, want_mode in ((0, 8, LIST), (n_sh, 8, SCAN), (1_000_000, 1, LIST), (12_000_000, 1, SCAN), (1_000_000, 8, SCAN)):
        passes = nq // 8 + (1 if nq % 8 >= 4 else 0) + (1 if (nq % 8) % 4 >= 2 else 0) + nq % 2
        rule = LIST if allowed == 0 or nq * (allowed * 68.0 * 2.0 + 1.2e6 * 68.0) <= passes * n_sh * 68.0 else SCAN
        assert rule == want_mode and pq_plan(n_sh, allowed, nq) == want_mode, (allowed, nq)
    # a shard below 1.2e6 codes always scans, whatever the index as a whole would do
    assert pq_plan(750, 10, 1) == SCAN and pq_plan(100_000_000, 10, 1) == LIST


NEW_SYMBOLS = ["mse_filter_slice", "mse_filter_concat", "mse_shard_group_filter", "mse_shard_group_filter_from_local",
               "mse_shard_group_live_filter", "mse_shard_filter_free", "mse_shard_filter_count", "mse_shard_filter_shard",
               "mse_shard_filter_global", "mse_shard_group_search_filtered", "mse_shard_group_search_filtered_dev",
               "mse_shard_group_pq_scan_topk_filtered", "mse_shard_group_query_topk_filtered", "mse_disk_query_topk_block_filtered",
               "mse_comm_search_filtered_dev", "mse_comm_pq_scan_topk_filtered", "mse_comm_query_topk_filtered"]


def test_new_entry_points_are_declared_exported_and_bound():
    import mse
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES, name
        assert getattr(ffi.lib(), name) is not None, name
    sig = ffi.SIGNATURES
    # every filtered call takes the arguments of the call it extends, plus the filter and the mode / regime
    assert len(sig["mse_shard_group_search_filtered"][1]) == len(sig["mse_shard_group_search"][1]) + 1
    assert len(sig["mse_shard_group_pq_scan_topk_filtered"][1]) == len(sig["mse_shard_group_pq_scan_topk"][1]) + 2
    assert len(sig["mse_shard_group_query_topk_filtered"][1]) == len(sig["mse_shard_group_query_topk"][1]) + 2
    assert len(sig["mse_disk_query_topk_block_filtered"][1]) == len(sig["mse_disk_query_topk_block"][1]) + 2
    assert len(sig["mse_comm_search_filtered_dev"][1]) == len(sig["mse_comm_search_dev"][1]) + 1
    assert len(sig["mse_comm_pq_scan_topk_filtered"][1]) == len(sig["mse_comm_pq_scan_topk"][1]) + 2
    assert len(sig["mse_comm_query_topk_filtered"][1]) == len(sig["mse_comm_query_topk"][1]) + 2
    for name in ("ShardFilter", "ShardGroup", "RowFilter", "Comm"):
        assert hasattr(mse, name)
    for cls, names in ((mse.RowFilter, ("slice", "concat")), (mse.ShardFilter, ("count", "shard", "to_global", "close")),
                       (mse.ShardGroup, ("filter", "filter_from_local", "live_filter", "bruteforce_topk_filtered",
                                         "bruteforce_topk_filtered_dev", "pq_scan_topk_filtered", "query_topk_filtered")),
                       (mse.Comm, ("search_filtered_dev", "pq_scan_topk_filtered", "query_topk_filtered"))):
        for n in names:
            assert hasattr(cls, n), (cls.__name__, n)
