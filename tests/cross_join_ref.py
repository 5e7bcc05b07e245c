"""Restatement of the cross join (include/mse.h mse_join_cross) and of the admission rule over its pair list (mse_pairs_admit), for the
tests: the pair list is the CPU oracle's score of every base row against each incoming row with filter and threshold applied; admission is
a plain Python walk (the handler's retain loop, src/query_disk_index.rs:513-527, over "allowed base rows first, all retained, then the
batch in row order"); the round count restates the synchronous integer rounds the device resolves the walk in."""
import numpy as np

NONE = 0xFFFFFFFF


def cross_pairs(orc, base, incoming, threshold, within=None):
    """(lo, hi, scores) in canonical order -- hi (the incoming row) ascending, then lo (the base row) ascending -- of the pairs whose base
    row the boolean mask `within` allows (shorter than the base: later rows excluded) and whose score, orc.score_all(base, incoming[hi])
    at lo, is >= threshold."""
    base = np.ascontiguousarray(base, np.uint16)
    incoming = np.ascontiguousarray(incoming, np.uint16)
    n = base.shape[0]
    ok = np.ones(n, bool)
    if within is not None:
        w = np.asarray(within, bool)
        ok = np.zeros(n, bool)
        ok[:min(n, w.size)] = w[:n]
    lo, hi, sc = [], [], []
    for j in range(incoming.shape[0]):
        if n == 0:
            break
        s = np.asarray(orc.score_all(base, incoming[j]), np.int64)
        for b in np.flatnonzero(ok & (s >= int(threshold))).tolist():
            lo.append(b)
            hi.append(j)
            sc.append(int(s[b]))
    return np.array(lo, np.uint32), np.array(hi, np.uint32), np.array(sc, np.int64)


def admit(m, cross_hi, cross_lo, among_lo=None, among_hi=None):
    """(kept bool [m], rep_base uint32 [m], rep_incoming uint32 [m]): incoming row j is kept iff it has no cross pair and no kept incoming
    row j' < j pairs with it among the incoming rows.  rep_base: the lowest base partner, NONE without one.  rep_incoming: j when kept, the
    lowest kept earlier neighbour when that dropped it, NONE when the base dropped it.  among_lo is None: only the base decides."""
    partners = [[] for _ in range(m)]
    for h, l in zip(np.asarray(cross_hi).tolist(), np.asarray(cross_lo).tolist()):
        partners[h].append(l)
    earlier = [[] for _ in range(m)]
    if among_lo is not None:
        for l, h in zip(np.asarray(among_lo).tolist(), np.asarray(among_hi).tolist()):
            assert l < h
            earlier[h].append(l)
    kept = np.zeros(m, bool)
    rep_base = np.full(m, NONE, np.uint32)
    rep_incoming = np.full(m, NONE, np.uint32)
    for j in range(m):
        if partners[j]:
            rep_base[j] = min(partners[j])
            continue                       # dropped by the base: it drops nobody
        kept_nb = [i for i in earlier[j] if kept[i]]
        if kept_nb:
            rep_incoming[j] = min(kept_nb)
        else:
            kept[j] = True
            rep_incoming[j] = j
    return kept, rep_base, rep_incoming


def admit_rounds(m, cross_hi, among_lo=None, among_hi=None):
    """(rounds, kept): the same rule as synchronous rounds over integer state (0 open, 1 kept, 2 dropped), started with the rows that have
    a cross pair already dropped: in a round an open row is dropped as soon as one earlier neighbour is kept and kept once all are
    dropped.  Without a list among the incoming rows every other row is kept at once and no round runs."""
    state = np.zeros(m, np.uint8)
    state[np.unique(np.asarray(cross_hi, np.int64))] = 2
    if among_lo is None:
        state[state == 0] = 1
        return 0, state == 1
    earlier = [[] for _ in range(m)]
    for l, h in zip(np.asarray(among_lo).tolist(), np.asarray(among_hi).tolist()):
        earlier[h].append(l)
    rounds = 0
    while (state == 0).any():
        nxt = state.copy()
        for j in np.flatnonzero(state == 0).tolist():
            ns = [int(state[i]) for i in earlier[j]]
            nxt[j] = 2 if 1 in ns else 0 if 0 in ns else 1
        state = nxt
        rounds += 1
    return rounds, state == 1
