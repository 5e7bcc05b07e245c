"""Grouped ("collapse") search, measured.  Not part of bench.py.

  python3 scripts/grouped_search_probe.py [--rows 1e7] [--reps 5]

On one MI355X, k = 10, 1 and 320 queries, MSE_MODE_MFMA: the whole grouped call for three groupings -- every row a group of its own,
runs of 8 rows, one group holding 90 % of the rows (a widened prefix answers it at k = 10) and one holding 99.9 % (the dense path) -- beside the ungrouped call at k = 10, the ungrouped
call at the first prefix's k', and the host alternative the grouped call replaces (ungrouped k = 1984, download, numpy collapse).  The
collapse kernel's own time and the dense path's split (score pass, group atomics, selection) come from the library's HIP events
(mse_searcher_grouped_timing).  Writes profiles/grouped_search_probe.json and prints it."""
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

GROUP_NONE = 0xFFFFFFFF


def timed(fn, reps):
    fn()   # warm: scratch allocated, code loaded
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def host_collapse(s, q, k, group_of):
    """What the grouped call replaces: over-fetch, download, walk on the host (a prefix of 1984 rows may still be too short)."""
    sc, ids = s.bruteforce_topk(q, 1984, mse.MODE_MFMA)
    out = []
    for i in range(ids.shape[0]):
        g = group_of[ids[i]].astype(np.int64)
        key = np.where(g == GROUP_NONE, (1 << 32) + ids[i].astype(np.int64), g)
        _, first = np.unique(key, return_index=True)
        out.append(np.sort(first)[:k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, k = int(a.rows), 10
    k1 = max(2 * k, k + 64)   # the first prefix (bruteforce.hip grouped_topk_dev)
    vecs = mse.VectorList.generate(0x5EED0001, 0, n)
    s = mse.Searcher(vecs)
    q = orc.gen_rows_f16(0x5EED0002, 0, 320)
    rng = np.random.default_rng(1)
    groupings = {
        "all_none": np.full(n, GROUP_NONE, np.uint32),
        "runs_of_8": (np.arange(n, dtype=np.uint32) // 8) * 8,
        "one_group_90pct": np.where(rng.random(n) < 0.9, 0, GROUP_NONE).astype(np.uint32),
        "one_group_99.9pct": np.where(rng.random(n) < 0.999, 0, GROUP_NONE).astype(np.uint32),
    }
    res = {"rows": n, "d": 1152, "k": k, "first_prefix": k1, "reps": a.reps, "mode": "mfma", "nq": {}}
    for nq in (1, 320):
        qq = q[:nq]
        row = {"ungrouped_k10_ms": timed(lambda: s.bruteforce_topk(qq, k, mse.MODE_MFMA), a.reps),
               "ungrouped_first_prefix_ms": timed(lambda: s.bruteforce_topk(qq, k1, mse.MODE_MFMA), a.reps),
               "grouped": {}}
        for name, group_of in groupings.items():
            g = mse.RowGroups(group_of)
            s.grouped_timing(2)
            ms = timed(lambda: s.bruteforce_topk(qq, k, mse.MODE_MFMA, groups=g), a.reps)
            ev = s.grouped_timing(0)
            calls = a.reps + 1
            row["grouped"][name] = {"call_ms": ms, "path_counts": s.grouped_stats(), "groups": g.count,
                                    "events_ms_per_call": {key: v / calls for key, v in ev.items()},
                                    "host_alternative_ms": timed(lambda: host_collapse(s, qq, k, group_of), max(a.reps // 2, 1))}
            g.close()
        res["nq"][str(nq)] = row
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "grouped_search_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
