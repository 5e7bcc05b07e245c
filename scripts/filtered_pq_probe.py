"""Filtered PQ flat scan, measured.  Not part of bench.py.

  python3 scripts/filtered_pq_probe.py [--rows 1e7] [--reps 5]

On one MI355X, random 64-byte codes with 4 descriptor bytes, r = 200, k = 10, batches of 1, 8 and 32 queries, allowed fractions 1, 0.5,
0.1, 0.01 and 1e-4 (random rows): the unfiltered batch call, the masked scan (mode "scan") and the id-list path (mode "list"), alternated
in one process; what mse_pq_filtered_plan picks at each point; and per batch size the allowed fraction at which the two measured curves
cross (log-log interpolation between the measured fractions), next to the fraction the plan function's byte-count rule implies.
Writes profiles/filtered_pq_probe.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "meme-search-engine_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  -- before libmse_hip.so
import mse  # noqa: E402
from oracle import orc  # noqa: E402
from conftest import make_pq  # noqa: E402

D = 1152
FRACTIONS = (1.0, 0.5, 0.1, 0.01, 1e-4)


def once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def crossing(fracs, list_ms, scan_ms):
    """the fraction at which list_ms == scan_ms, between the two neighbouring measured fractions where the sign changes (log-log)"""
    d = [np.log(a) - np.log(b) for a, b in zip(list_ms, scan_ms)]
    for i in range(len(fracs) - 1):
        if d[i] > 0 >= d[i + 1]:                     # fractions descend: list slower at fracs[i], not slower at fracs[i + 1]
            t = d[i] / (d[i] - d[i + 1])
            return float(np.exp(np.log(fracs[i]) + t * (np.log(fracs[i + 1]) - np.log(fracs[i]))))
    return None                                      # one path wins everywhere that was measured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, r, k = int(a.rows), 200, 10
    rng = np.random.default_rng(3)
    cents, T, dpc, _ = make_pq(orc)
    pq = mse.ProductQuantizer(cents, T, dpc, D)
    codes = mse.Codes(rng.integers(0, 256, size=(n, 64), dtype=np.uint8), rng.integers(0, 256, size=(n, 4), dtype=np.uint8))
    scales = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)
    qs = (rng.standard_normal((32, D)) / np.sqrt(D)).astype(np.float32)
    res = {"rows": n, "r": r, "k": k, "reps": a.reps, "points": [], "crossover": {}}
    for nq in (1, 8, 32):
        q = qs[:nq]
        per = {"list": [], "scan": []}
        for frac in FRACTIONS:
            f = mse.RowFilter(np.ones(n, bool) if frac == 1.0 else rng.random(n) < frac)
            calls = {"unfiltered": lambda: pq.scan_topk_batch(codes, q, r, k, None, scales),
                     "scan": lambda: pq.scan_topk_batch_filtered(codes, f, q, r, k, None, scales, "scan"),
                     "list": lambda: pq.scan_topk_batch_filtered(codes, f, q, r, k, None, scales, "list")}
            ms = {name: [] for name in calls}
            unc = {}
            for name, fn in calls.items():
                fn()                                 # warm: scratch allocated, code loaded
                unc[name] = pq.last_uncertified
            for _ in range(a.reps):                  # alternated, so that clock and power drift fall on all alike
                for name, fn in calls.items():
                    ms[name].append(once(fn))
            med = {name: float(np.median(v)) for name, v in ms.items()}
            res["points"].append({"nq": nq, "fraction": frac, "allowed": f.count, "ms": med, "uncertified": unc,
                                  "scan_over_unfiltered": med["scan"] / med["unfiltered"], "list_over_scan": med["list"] / med["scan"],
                                  "list_over_unfiltered": med["list"] / med["unfiltered"], "plan_picks": pq.filtered_plan(n, f.count, nq)})
            per["list"].append(med["list"])
            per["scan"].append(med["scan"])
            f.close()
        lo, hi = 0, n                                # the plan function's own boundary, by bisection over its answers
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if pq.filtered_plan(n, mid, nq) == "list" else (lo, mid)
        res["crossover"][str(nq)] = {"measured_fraction": crossing(FRACTIONS, per["list"], per["scan"]), "plan_fraction": lo / n}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "filtered_pq_probe.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
