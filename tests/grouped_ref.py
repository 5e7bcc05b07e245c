"""Numpy reference of the grouped search (include/mse.h mse_groups), shared by tests/test_grouped_host.py and tests/test_gpu_grouped.py:
the collapse of a ranked id list, and the grouped top-k from all scores of a query."""
import numpy as np

GROUP_NONE = 0xFFFFFFFF
ID_NONE = 0xFFFFFFFF
I64_MIN = np.iinfo(np.int64).min


def collapse_positions(ranked_ids, group_of):
    """Positions (ascending) of the representatives in a ranked list of row ids, best first: an entry is one if no earlier entry has
    its group.  A row of group GROUP_NONE, or at / past len(group_of), is a group of its own."""
    ranked_ids = np.asarray(ranked_ids, np.int64)
    group_of = np.asarray(group_of, np.int64)
    g = np.full(ranked_ids.size, GROUP_NONE, np.int64)
    inside = ranked_ids < group_of.size
    g[inside] = group_of[ranked_ids[inside]]
    # a key no group id can take for the rows that are groups of their own: ids are below 2^32
    key = np.where(g == GROUP_NONE, (1 << 32) + ranked_ids, g)
    _, first = np.unique(key, return_index=True)
    return np.sort(first)


def grouped_topk(scores, group_of, k, allowed=None):
    """(scores [k] i64, ids [k] u32) of one query: the eligible rows (`allowed`: a boolean mask, or None for all) in (score desc, id asc)
    order, collapsed, the first k, padded with INT64_MIN / ID_NONE."""
    scores = np.asarray(scores, np.int64)
    ids = np.arange(scores.size) if allowed is None else np.flatnonzero(allowed)
    sc = scores[ids]
    order = np.lexsort((ids, _neg_key(sc)))
    ranked, ranked_sc = ids[order], sc[order]
    keep = collapse_positions(ranked, group_of)[:k]
    out_s = np.full(k, I64_MIN, np.int64)
    out_i = np.full(k, ID_NONE, np.uint32)
    out_s[:keep.size] = ranked_sc[keep]
    out_i[:keep.size] = ranked[keep]
    return out_s, out_i


def _neg_key(sc):
    """A key that sorts ascending where the i64 scores sort descending, exact for every value (-INT64_MIN does not exist in i64)."""
    return np.uint64(0xFFFFFFFFFFFFFFFF) - (sc.view(np.uint64) ^ np.uint64(0x8000000000000000))
