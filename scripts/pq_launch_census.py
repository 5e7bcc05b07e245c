#!/usr/bin/env python3
"""Launch census of the PQ flat scan's host path: one call of every shape, to be run under a kernel trace --

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/pq_launch_census.py

once per library (MSE_HIP_LIB selects it), each run in a process of its own.  Two libraries whose host paths make the same launches
give equal calls-per-kernel tables:

    python scripts/pq_launch_census.py --tables parent=DIR/.../NAME_kernel_stats.csv new=... > profiles/pq_host_path_census.json

The shapes: 1, 2, 3, 4, 8, 9 and 32 queries per call, with and without a re-scoring Searcher, unfiltered and filtered in SCAN and LIST
mode, and one batch over tied codes whose every certificate fails (each query repeated through the exact scan)."""
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "meme-search-engine_amd")):
    sys.path.insert(0, p)

N, D, R, K = 200_000, 1152, 200, 10
BATCHES = (1, 2, 3, 4, 8, 9, 32)


def tables(args):
    out = {}
    for a in args:
        name, path = a.split("=", 1)
        with open(path, newline="") as fh:
            out[name] = {row["Name"]: int(row["Calls"]) for row in csv.DictReader(fh)}
    names = list(out)
    out["equal"] = all(out[n] == out[names[0]] for n in names)
    print(json.dumps(out, indent=1, sort_keys=True))
    return 0 if out["equal"] else 1


def main():
    import numpy as np
    import torch  # noqa: F401  (before libmse_hip.so: one HIP runtime per process)
    import mse
    from mse import ffi
    rng = np.random.default_rng(20)
    T = np.linalg.qr(rng.standard_normal((D, D)))[0].astype(np.float32)
    cents = (rng.standard_normal((256, D)) / np.sqrt(D)).astype(np.float32)
    pq = mse.ProductQuantizer(cents, T, 18, D)
    codes = mse.Codes(rng.integers(0, 256, size=(N, 64), dtype=np.uint8), rng.integers(0, 256, size=(N, 4), dtype=np.uint8))
    tied = mse.Codes(np.tile(rng.integers(0, 256, size=(1, 64), dtype=np.uint8), (N, 1)), np.zeros((N, 4), np.uint8))
    scales = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)
    searcher = mse.Searcher(mse.VectorList.generate(0x5EED0001, 0, N))
    qs = (rng.standard_normal((32, D)) / np.sqrt(D)).astype(np.float32)
    f = mse.RowFilter(rng.random(N) < 0.3)
    calls = 0
    for s in (None, searcher):
        for nq in BATCHES:
            pq.scan_topk_batch(codes, qs[:nq], R, K, s, scales)
            for mode in ("scan", "list"):
                pq.scan_topk_batch_filtered(codes, f, qs[:nq], R, K, s, scales, mode)
            calls += 3
    pq.scan_topk_batch(tied, qs[:8], R, K, searcher, scales)
    uncertified = pq.last_uncertified
    assert uncertified == 8, uncertified
    print(json.dumps({"calls": calls + 1, "uncertified_in_the_tied_batch": uncertified, "library": os.path.basename(os.path.dirname(ffi.LIB_PATH)) + "/" + os.path.basename(ffi.LIB_PATH)}))
    return 0


if __name__ == "__main__":
    sys.exit(tables(sys.argv[2:]) if len(sys.argv) > 1 and sys.argv[1] == "--tables" else main())
