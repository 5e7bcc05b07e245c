"""Numpy reference of the grouped graph search (include/mse.h "grouped graph search"), shared by tests/test_grouped_graph_host.py and
tests/test_gpu_grouped_graph.py.  The rule has two statements:
  1. per group, the best record by (score desc, id asc) stays and every other record of the group leaves the list (what the device's
     group step does over an UNRANKED visited list, in place);
  2. in the list ranked by (score desc, id asc) a record is kept if no earlier record has its group (grouped_ref.collapse_positions).
A record whose row has group GROUP_NONE, or lies at / past the grouping, is a group of its own; a hole (ID_NONE, INT64_MIN) is no record."""
import numpy as np

from grouped_ref import GROUP_NONE, I64_MIN, ID_NONE, _neg_key, collapse_positions


def group_step(ids, scores, n_visited, group_of):
    """Statement 1 over one list: (ids, scores) copies in which every grouped live record among the first min(n_visited, len) that is
    not its group's best by (score desc, id asc) has become a hole; everything else -- holes, ungrouped records, entries at or past
    n_visited -- is as it was and where it was."""
    ids, scores = np.array(ids, np.uint32), np.array(scores, np.int64)
    group_of = np.asarray(group_of, np.uint32)
    n = min(int(n_visited), ids.size)
    pos = np.arange(n)
    head = ids[:n].astype(np.int64)
    live = pos[(head != ID_NONE) & (head < group_of.size)]
    live = live[group_of[head[live]] != GROUP_NONE]
    g = group_of[head[live]]
    order = np.lexsort((head[live], _neg_key(scores[live]), g))   # by group, then score desc, then id asc
    gs = g[order]
    first = np.ones(order.size, bool)
    first[1:] = gs[1:] != gs[:-1]
    losers = live[order][~first]
    ids[losers], scores[losers] = ID_NONE, I64_MIN
    return ids, scores


def ranked(ids, scores, n_visited=None):
    """The live records of a list in the request path's total order (score desc, id asc): (ids, scores)"""
    ids, scores = np.asarray(ids, np.uint32), np.asarray(scores, np.int64)
    n = ids.size if n_visited is None else min(int(n_visited), ids.size)
    ids, scores = ids[:n], scores[:n]
    keep = ids != ID_NONE
    ids, scores = ids[keep], scores[keep]
    order = np.lexsort((ids, _neg_key(scores)))
    return ids[order], scores[order]


def cut(ids, scores, k):
    """the first k of a ranked list, padded with ID_NONE / INT64_MIN"""
    out_i, out_s = np.full(k, ID_NONE, np.uint32), np.full(k, I64_MIN, np.int64)
    m = min(k, len(ids))
    out_i[:m], out_s[:m] = ids[:m], scores[:m]
    return out_i, out_s


def grouped_cut(ids, scores, group_of, k, n_visited=None):
    """Statement 2, the contract's numpy restatement: rank the visited list, keep the first record of every group, take the first k:
    (ids [k], scores [k])"""
    r_ids, r_sc = ranked(ids, scores, n_visited)
    keep = collapse_positions(r_ids, group_of)
    return cut(r_ids[keep], r_sc[keep], k)
