"""Grouped search on the shard group, measured.  Not part of bench.py; no figure here gates anything.

  python3 scripts/sharded_grouped_probe.py [--rows 2e7] [--shards 8] [--queries 32,320] [--k 10] [--reps 7]

On one MI355X, `shards` logical shards on device 0 over `rows` x 1152 generated rows, grouped in runs of 1 .. 40 consecutive rows
(frames of one video).
  slicing   mse_shard_group_groups -- every shard's part cut and relabelled on the device, plus the copy of the global labels for the
            merge -- against the host route it replaces: the labels downloaded, each shard's rows relabelled in numpy, one upload per shard.
  searching bruteforce_topk_grouped next to the ungrouped bruteforce_topk, alternated in one process: median of `reps` rounds after one
            warm round of the wall time and of mse_shard_group_last_timing's phases.  "merge_ms" of the grouped call includes the group
            step; the ungrouped call's is the plain merge it is reported against.
Writes profiles/sharded_grouped_probe.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  -- before libmse_hip.so
import mse  # noqa: E402
from oracle import orc  # noqa: E402

D = 1152
SEED_BASE, SEED_QUERY = 0x5EED0001, 0x5EED0002
NONE = 0xFFFFFFFF


def wall_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def frames(n, seed):
    """runs of 1 .. 40 consecutive rows, each labelled by its first row"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 41, size=n // 20 + 64)
    while lengths.sum() < n:
        lengths = np.concatenate([lengths, rng.integers(1, 41, size=n // 20 + 64)])
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return np.repeat(starts, lengths)[:n].astype(np.uint32)


def host_slice(labels, lo, hi):
    """the canonical relabelling in numpy: a grouped row's label is the local id of the first row of its group inside the slice"""
    part = labels[lo:hi]
    _, first, inv = np.unique(part, return_index=True, return_inverse=True)
    out = first[inv].astype(np.uint32)
    out[part == NONE] = NONE
    return out


def median_of(rows):
    return {key: float(np.median([r[key] for r in rows])) for key in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=2e7)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--queries", default="32,320")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, G, k = int(a.rows), a.shards, a.k
    grp = mse.ShardGroup(G, D, devices=[0] * G)
    grp.generate(SEED_BASE, 0, n)
    labels = frames(n, 6)
    rg = mse.RowGroups(labels)
    bounds = [mse.shard_range(n, g, G) for g in range(G)]

    def host_route():
        host = rg.to_host()
        return [mse.RowGroups(host_slice(host, lo, hi)) for lo, hi in bounds]
    dev, host = [], []
    sg = None
    for rep in range(a.reps + 1):
        if sg is not None:
            sg.close()
        t, sg = wall_ms(lambda: grp.groups(rg))
        dev.append(t)
        t, parts = wall_ms(host_route)
        host.append(t)
        if rep == a.reps:
            for g, p in enumerate(parts):
                assert np.array_equal(p.to_host(), sg.shard(g).to_host()) and p.count == sg.shard(g).count
        for p in parts:
            p.close()
    res = {"rows": n, "shards": G, "k": k, "reps": a.reps, "groups": rg.count,
           "slicing": {"device_ms": float(np.median(dev[1:])), "host_route_ms": float(np.median(host[1:]))}, "searching": {}}
    for nq in [int(x) for x in a.queries.split(",")]:
        q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
        grouped, plain = [], []
        for rep in range(a.reps + 1):
            t, (gs, gi) = wall_ms(lambda: grp.bruteforce_topk_grouped(sg, q, k))
            grouped.append(dict(grp.last_timing(), call_ms=t))
            t, (ps, pi) = wall_ms(lambda: grp.bruteforce_topk(q, k))
            plain.append(dict(grp.last_timing(), call_ms=t))
        assert (gi != NONE).all() and all(len(set(labels[row].tolist())) == k for row in gi), "one result per group"
        assert np.array_equal(gi[:, 0], pi[:, 0]) and np.array_equal(gs[:, 0], ps[:, 0]), "the best row leads both answers"
        res["searching"][str(nq)] = {"grouped": median_of(grouped[1:]), "ungrouped": median_of(plain[1:]),
                                     "paths_shard0": dict(zip(("prefix", "widened", "dense"), grp.searcher(0).grouped_stats()))}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sharded_grouped_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    sg.close()
    rg.close()
    grp.close()


if __name__ == "__main__":
    main()
