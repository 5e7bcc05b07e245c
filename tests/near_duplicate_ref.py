"""Restatement of the near-duplicate join (include/mse.h mse_join_self) and of the keep-first rule over its pair list, for the tests:
the pair list is the all-pairs score matrix of the CPU oracle with band, filter and threshold applied; the keep-first walk is a plain
Python loop (the handler's retain loop, src/query_disk_index.rs:513-527, in row order); the labels come from the walk."""
import numpy as np

NONE = 0xFFFFFFFF


def score_matrix(orc, base):
    """S[i][j] = fast_dot(row j, row i) as the oracle's score_all gives it with row i as the query (int64 [n][n])."""
    base = np.ascontiguousarray(base, np.uint16)
    n = base.shape[0]
    s = np.empty((n, n), np.int64)
    for i in range(n):
        s[i] = orc.score_all(base, base[i])
    return s


def pairs_from_scores(s, threshold, window=0, within=None):
    """(lo, hi, scores) in canonical order -- hi ascending, then lo ascending -- of the pairs lo < hi with hi - lo <= window (0: no
    limit), both rows allowed by the boolean mask `within` (shorter than n: later rows excluded) and s[hi][lo] >= threshold."""
    s = np.asarray(s)
    n = s.shape[0]
    ok = np.ones(n, bool)
    if within is not None:
        w = np.asarray(within, bool)
        ok = np.zeros(n, bool)
        ok[:min(n, w.size)] = w[:n]
    lo, hi, sc = [], [], []
    for h in range(n):
        if not ok[h]:
            continue
        first = 0 if window == 0 else max(0, h - int(window))
        for l in range(first, h):
            if ok[l] and int(s[h, l]) >= int(threshold):
                lo.append(l)
                hi.append(h)
                sc.append(int(s[h, l]))
    return np.array(lo, np.uint32), np.array(hi, np.uint32), np.array(sc, np.int64)


def keep_first(n, lo, hi):
    """(kept bool [n], rep uint32 [n]): row i is kept iff no kept row j < i forms a pair with it; rep is the row itself when kept, the
    lowest kept earlier neighbour when dropped."""
    earlier = [[] for _ in range(n)]
    for l, h in zip(lo.tolist(), hi.tolist()):
        earlier[h].append(l)
    kept = np.zeros(n, bool)
    rep = np.arange(n, dtype=np.uint32)
    for i in range(n):
        kept_nb = [j for j in earlier[i] if kept[j]]
        if kept_nb:
            rep[i] = min(kept_nb)
        else:
            kept[i] = True
    return kept, rep


def labels(kept, rep):
    """Group labels: rep[i] for every row of a group of two or more (the representative included), NONE for every other row."""
    n = len(rep)
    out = np.full(n, NONE, np.uint32)
    dropped = np.flatnonzero(~kept)
    out[dropped] = rep[dropped]
    heads = np.unique(rep[dropped])
    out[heads] = heads
    return out
