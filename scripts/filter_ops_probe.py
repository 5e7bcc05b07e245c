"""Row filters as values, measured.  Not part of bench.py.

  python3 scripts/filter_ops_probe.py [--rows 1e8] [--score-rows 1e7] [--reps 5]

On one MI355X: `rows` rows with 4 descriptor bytes each (random), and a generated f16 base of `score-rows` x 1152 for the score threshold
(1e8 x 1152 f16 rows are 230 GB; the threshold pass itself reads 8 B per row and does not care about the width).  For from_descriptors,
combine (AND), not, from_scores and to_bits: the wall time of the whole call (median of `reps`), next to the host route it replaces -- a
numpy pass over a host copy of the same data -> numpy.packbits -> mse_filter_from_bits, for the scores Searcher.scores -> numpy first.
Per new kernel: its own HIP-event time (mse_filter_kernel_timing), the bytes it must move, and that rate against the 6.29 TB/s copy rate
of the part.  Writes profiles/filter_ops_probe.json and prints it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  -- before libmse_hip.so
import mse  # noqa: E402
from mse import ffi  # noqa: E402
from oracle import orc  # noqa: E402

D = 1152
COPY_RATE = 6.29e12


def timed(fn, reps):
    """(median wall ms, median kernel ms by the library's hook, the last result) of fn over reps calls after one warm call"""
    L = ffi.lib()
    r = fn()
    wall, kern = [], []
    for _ in range(reps):
        if hasattr(r, "close"):
            r.close()
        L.mse_filter_kernel_timing(2, None)
        t0 = time.perf_counter()
        r = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms = C.c_double()
        L.mse_filter_kernel_timing(0, C.byref(ms))
        kern.append(ms.value)
    return float(np.median(wall)), float(np.median(kern)), r


def kernel_entry(ms, nbytes):
    rate = nbytes / (ms * 1e-3) if ms > 0 else 0.0
    return {"kernel_ms": ms, "bytes": int(nbytes), "GBps": rate / 1e9, "of_copy_rate": rate / COPY_RATE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--score-rows", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, ns, reps = int(a.rows), int(a.score_rows), a.reps
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    codes = mse.Codes(np.zeros((n, 1), np.uint8), desc)
    ranges = {0: (64, 255), 3: (0, 127)}                                    # "channel 0 >= 64 and time bucket <= 127": 3/8 of the rows
    words = n / 32 * 4
    res = {"rows": n, "score_rows": ns, "reps": reps, "copy_rate_GBps": COPY_RATE / 1e9, "ops": {}}

    def host_desc():
        return mse.RowFilter((desc[:, 0] >= 64) & (desc[:, 3] <= 127))
    dev_ms, k_ms, fa = timed(lambda: mse.RowFilter.from_descriptors(codes, ranges), reps)
    host_ms, _, fh = timed(host_desc, reps)
    assert fa.count == fh.count
    res["ops"]["from_descriptors"] = {"device_ms": dev_ms, "host_route_ms": host_ms, "allowed": fa.count, **kernel_entry(k_ms, n * 4 + words)}
    fh.close()

    mask_a = fa.to_mask()
    mask_b = rng.random(n) < 0.5
    fb = mse.RowFilter(mask_b)
    dev_ms, k_ms, fc = timed(lambda: fa & fb, reps)
    host_ms, _, fh = timed(lambda: mse.RowFilter(mask_a & mask_b), reps)
    assert fc.count == fh.count
    res["ops"]["combine"] = {"device_ms": dev_ms, "host_route_ms": host_ms, "allowed": fc.count, **kernel_entry(k_ms, 3 * words)}
    fh.close()
    fc.close()

    dev_ms, k_ms, fc = timed(lambda: ~fa, reps)
    host_ms, _, fh = timed(lambda: mse.RowFilter(~mask_a), reps)
    assert fc.count == fh.count
    res["ops"]["not"] = {"device_ms": dev_ms, "host_route_ms": host_ms, "allowed": fc.count, **kernel_entry(k_ms, 2 * words)}
    fh.close()
    fc.close()

    L = ffi.lib()
    bits = np.empty((n + 7) // 8, np.uint8)
    wall = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        ffi.check(L.mse_filter_to_bits(fa._h, bits.ctypes.data_as(ffi.u8p)), "to_bits")
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    fa.to_mask()
    res["ops"]["to_bits"] = {"device_ms": float(np.median(wall[1:])), "bytes": int(bits.size), "to_mask_ms": (time.perf_counter() - t0) * 1e3}
    for f in (fa, fb):
        f.close()
    codes.close()
    del desc, mask_a, mask_b

    vecs = mse.VectorList.generate(0x5EED0001, 0, ns)
    s = mse.Searcher(vecs)
    q = orc.gen_rows_f16(0x5EED0002, 0, 1)[0]
    sc = s.scores(q)
    thr = int(np.sort(sc)[-1000])                                            # the thousand best rows
    dev_ms, k_ms, fc = timed(lambda: mse.RowFilter.from_scores(s, q, thr), reps)
    host_ms, _, fh = timed(lambda: mse.RowFilter(s.scores(q) >= thr), reps)
    assert fc.count == fh.count == int((sc >= thr).sum())
    res["ops"]["from_scores"] = {"device_ms": dev_ms, "host_route_ms": host_ms, "allowed": fc.count, **kernel_entry(k_ms, ns * 8 + ns / 8)}

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "filter_ops_probe.json"), "w") as fh_:
        json.dump(res, fh_, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
