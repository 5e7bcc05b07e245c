"""Row filters on the shard group, measured.  Not part of bench.py; no figure here gates anything.

  python3 scripts/sharded_filter_probe.py [--filter-rows 1e8] [--rows 2e7] [--shards 8] [--queries 32] [--reps 5]

On one MI355X, `shards` logical shards on device 0.
  slicing   a group of `filter-rows` rows (64-wide rows: only the row COUNT matters to a filter) and a random global filter at 0.5:
            mse_shard_group_filter -- every shard's slice cut on the device -- against the host route it replaces: to_bits of the global
            filter, the shards' rows sliced in numpy, mse_filter_from_bits per shard.  The default split starts shards at rows that are no
            multiple of 32 whenever filter-rows / shards is none.
  searching a group of `rows` x 1152 generated rows and one unsharded base of the same rows: bruteforce_topk_filtered at allowed
            fractions 1, 0.5 and 1e-4 next to the unfiltered sharded call and the unsharded filtered call, alternated in one process
            (median wall ms of `reps` rounds after one warm round).
Writes profiles/sharded_filter_probe.json and prints it."""
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


def wall_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def slicing(n, G, reps):
    grp = mse.ShardGroup(G, 64, devices=[0] * G)
    grp.generate(SEED_BASE, 0, n)
    mask = np.random.default_rng(4).random(n) < 0.5
    rf = mse.RowFilter(mask)
    bounds = [mse.shard_range(n, g, G) for g in range(G)]

    def host_route():
        m = rf.to_mask()
        return grp.filter_from_local([mse.RowFilter(m[lo:hi]) for lo, hi in bounds])
    dev, host = [], []
    for rep in range(reps + 1):
        t, sf = wall_ms(lambda: grp.filter(rf))
        dev.append(t)
        t, sh = wall_ms(host_route)
        host.append(t)
        assert sf.count == sh.count == rf.count
        if rep == reps:
            back = sf.to_global()
            assert back.count == rf.count and np.array_equal(back.to_mask(), mask)
            back.close()
        sf.close()
        sh.close()
    out = {"rows": n, "shards": G, "first_rows": [lo for lo, _ in bounds], "allowed": rf.count,
           "device_ms": float(np.median(dev[1:])), "host_route_ms": float(np.median(host[1:]))}
    rf.close()
    grp.close()
    return out


def searching(n, G, nq, k, reps):
    q = orc.gen_rows_f16(SEED_QUERY, 0, nq)
    grp = mse.ShardGroup(G, D, devices=[0] * G)
    grp.generate(SEED_BASE, 0, n)
    whole = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, n))
    rng = np.random.default_rng(5)
    fracs = {"1": np.ones(n, bool), "0.5": rng.random(n) < 0.5, "1e-4": rng.random(n) < 1e-4}
    filters = {name: mse.RowFilter(m) for name, m in fracs.items()}
    shard_filters = {name: grp.filter(f) for name, f in filters.items()}
    times = {"sharded_unfiltered": []}
    for name in fracs:
        times["sharded_filtered_" + name] = []
        times["unsharded_filtered_" + name] = []
    for rep in range(reps + 1):
        t, ref = wall_ms(lambda: grp.bruteforce_topk(q, k))
        times["sharded_unfiltered"].append(t)
        for name in fracs:
            t, a = wall_ms(lambda: grp.bruteforce_topk_filtered(shard_filters[name], q, k))
            times["sharded_filtered_" + name].append(t)
            t, b = wall_ms(lambda: whole.bruteforce_topk(q, k, allow=filters[name]))
            times["unsharded_filtered_" + name].append(t)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
            if name == "1":
                assert np.array_equal(a[0], ref[0]) and np.array_equal(a[1], ref[1])
    out = {"rows": n, "shards": G, "queries": nq, "k": k, "allowed": {name: f.count for name, f in filters.items()},
           "ms": {name: float(np.median(v[1:])) for name, v in times.items()}}
    for x in list(shard_filters.values()) + list(filters.values()):
        x.close()
    grp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter-rows", type=float, default=1e8)
    ap.add_argument("--rows", type=float, default=2e7)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--queries", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {"reps": a.reps, "slicing": slicing(int(a.filter_rows), a.shards, a.reps),
           "searching": searching(int(a.rows), a.shards, a.queries, a.k, a.reps)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sharded_filter_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
