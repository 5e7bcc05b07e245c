"""Filtered brute-force search, measured (filtered search).  Not part of bench.py.

  python3 scripts/filtered_scan_probe.py [--rows 1e8] [--reps 5]

On one MI355X: (1) the unfiltered and the 50 %-filtered 320-query MFMA pass over the rows, alternated in one process;
(2) one query through the sparse path (the filter's id list scored directly) at 1e3 / 1e4 / 1e5 allowed rows, against the masked
scan for the same query and filter; (3) both paths around the crossover rule of the auto mode.  Writes profiles/filtered_scan_probe.json and prints it."""
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


def timed(fn, reps):
    fn()   # warm: scratch allocated, code loaded
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = int(a.rows)
    vecs = mse.VectorList.generate(0x5EED0001, 0, n)
    s = mse.Searcher(vecs)
    q = orc.gen_rows_f16(0x5EED0002, 0, 320)
    rng = np.random.default_rng(1)
    half = mse.RowFilter(rng.random(n) < 0.5)
    res = {"rows": n, "d": 1152, "reps": a.reps, "pass_320_ms": {"unfiltered": [], "filtered_50pct": []}}
    # alternated, so that clock and power drift fall on both alike
    for _ in range(a.reps):
        res["pass_320_ms"]["unfiltered"] += timed(lambda: s.bruteforce_topk(q, 10, mse.MODE_MFMA), 1)
        res["pass_320_ms"]["filtered_50pct"] += timed(lambda: s.bruteforce_topk(q, 10, mse.MODE_MFMA, allow=half), 1)
    half.close()
    med = {k: float(np.median(v)) for k, v in res["pass_320_ms"].items()}
    res["pass_320_median_ms"] = med
    res["filtered_over_unfiltered"] = med["filtered_50pct"] / med["unfiltered"]
    res["sparse_1q_ms"] = {}
    for count in (1000, 10000, 100000):
        f = mse.RowFilter(np.sort(rng.choice(n, count, replace=False)).astype(np.uint32), n_rows=n)
        sp = timed(lambda: s.bruteforce_topk(q[:1], 10, mse.MODE_EXACT, allow=f), a.reps)
        sc = timed(lambda: s.bruteforce_topk(q[:1], 10, mse.MODE_MFMA, allow=f), a.reps)
        res["sparse_1q_ms"][str(count)] = {"sparse": float(np.median(sp)), "masked_scan": float(np.median(sc)),
                                           "speedup": float(np.median(sc) / np.median(sp))}
        f.close()
    # the crossover: the id-list pass (MODE_EXACT) against the masked scan (MODE_MFMA) around the boundary of the rule in bruteforce.hip
    # (filter_sparse: count x ceil(nq / 8) x 3 <= rows x ceil(nq / pass width) x 2), and what the rule picks
    tile = mse.ffi.lib().mse_queries_per_pass_max(1152)
    res["crossover"] = []
    for frac in (1 / 256, 1 / 64, 1 / 32, 1 / 16, 1 / 8):
        f = mse.RowFilter(rng.random(n) < frac)
        for nq in (9, 64, 320):
            lst = timed(lambda: s.bruteforce_topk(q[:nq], 10, mse.MODE_EXACT, allow=f), 2)
            scn = timed(lambda: s.bruteforce_topk(q[:nq], 10, mse.MODE_MFMA, allow=f), 2)
            rule = f.count * ((nq + 7) // 8) * 3 <= n * ((nq + tile - 1) // tile) * 2
            res["crossover"].append({"count": f.count, "nq": nq, "list_ms": float(np.median(lst)), "scan_ms": float(np.median(scn)),
                                     "rule_picks": "list" if rule else "scan"})
        f.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "filtered_scan_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
