"""The near-duplicate join, measured.  Not part of bench.py, not a test.

  python3 scripts/near_duplicate_probe.py [--runs 1e6:0,1e7:2097152] [--dup 0.02] [--threshold 0.95] [--sample 16]

On one MI355X: the hard set of bench_ann.py (no micro-clusters) with a planted duplicate fraction -- `dup` of the rows are overwritten by
a noisy copy of an earlier row -- joined in MSE_MODE_MFMA per run `rows:window`.  Per run: the wall time of the call and of the keep-first
resolution, the HIP-event time of the tile launches, the re-score and the list build (mse_join_timing), the tile kernel's TFLOP/s
(2 x 128 x 128 x 1152 flop per tile that did work) as a fraction of the 2500 TFLOP/s f16 MFMA peak and against the 320-query scan's rate
on the same box in the same run, pairs nominated against pairs kept, and -- the comparison that counts -- what the same answer costs
without the join: one RowFilter.from_scores call per row, timed on `sample` rows and scaled to all of them.
Writes profiles/near_duplicate_probe.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  -- before libmse_hip.so
import mse  # noqa: E402
import bench_ann  # noqa: E402

D = 1152
MFMA_PEAK_TFLOPS = 2500.0
TILE = 128


def planted_base(n, dup, seed=5):
    """[n, 1152] f16 device tensor of the hard set; a fraction `dup` of the rows replaced by near-copies of earlier rows"""
    hs = bench_ann.HardSet(n, **bench_ann.HARD_PARAMS)
    rows = hs.rows(n, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    m = int(n * dup)
    dst = torch.randperm(n - 1, device="cuda", generator=g)[:m] + 1
    src = (torch.rand(m, device="cuda", generator=g) * dst.float()).long().clamp_(max=n - 2)
    src = torch.minimum(src, dst - 1)
    for i in range(0, m, 1 << 16):
        x = rows[src[i:i + (1 << 16)]].float() + torch.randn(min(1 << 16, m - i), D, device="cuda", generator=g) * (0.1 / D ** 0.5)
        rows[dst[i:i + (1 << 16)]] = (x / x.norm(dim=1, keepdim=True)).half()
    torch.cuda.synchronize()
    return rows, m


def scan_rate(s, rows, n):
    """PFLOP/s of the 320-query MFMA scan over the same rows (HIP events around the scan kernel)"""
    q = rows[:320].cpu().numpy().view(np.uint16)
    s.bruteforce_topk(q, 10, mse.MODE_MFMA)
    s.scan_timing(2)
    s.bruteforce_topk(q, 10, mse.MODE_MFMA)
    ms, launches = s.scan_timing(0)
    return (2.0 * n * D * 320 / (ms * 1e-3) / 1e15) if ms > 0 else None


def one_run(n, window, dup, threshold, sample):
    rows, planted = planted_base(n, dup)
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
    s = mse.Searcher(vecs)
    thr = mse.scale_dot_result(threshold)
    out = {"rows": n, "window": window, "planted_rows": planted, "threshold": threshold}
    out["scan_320_PFLOPs"] = scan_rate(s, rows, n)
    s.join_timing(1)
    t0 = time.perf_counter()
    pairs = s.near_duplicates(thr, window=window, mode=mse.MODE_MFMA)
    out["join_wall_s"] = time.perf_counter() - t0
    tm, st = s.join_timing(0), s.join_stats()
    flop = st["tiles"] * 2.0 * TILE * TILE * D
    tflops = flop / (tm["tile_ms"] * 1e-3) / 1e12 if tm["tile_ms"] > 0 else None
    out.update({"tile_kernel_s": tm["tile_ms"] / 1e3, "rescore_s": tm["rescore_ms"] / 1e3, "list_build_s": tm["list_ms"] / 1e3, "tiles": st["tiles"],
                "tile_TFLOPs": tflops, "tile_of_f16_mfma_peak": tflops / MFMA_PEAK_TFLOPS if tflops else None,
                "tile_of_scan_320_rate": tflops / 1e3 / out["scan_320_PFLOPs"] if tflops and out["scan_320_PFLOPs"] else None,
                "pairs_nominated": st["nominated"], "pairs_kept": st["kept"], "strips_repeated": st["strips_repeated"]})
    t0 = time.perf_counter()
    dupf = pairs.duplicates()
    out["resolution_wall_s"] = time.perf_counter() - t0
    out["resolution_rounds"] = s.join_stats()["rounds"]
    out["rows_dropped"] = dupf.count
    # the parent's route to the same answer: one from_scores call per row
    ids = np.random.default_rng(1).integers(0, n, sample)
    host = rows[torch.from_numpy(ids).cuda()].cpu().numpy().view(np.uint16)
    mse.RowFilter.from_scores(s, host[0], thr).close()
    t0 = time.perf_counter()
    for r in host:
        mse.RowFilter.from_scores(s, r, thr).close()
    per_row = (time.perf_counter() - t0) / sample
    out["from_scores_per_row_s"] = per_row
    out["from_scores_all_rows_s_scaled"] = per_row * n
    out["join_speedup_over_from_scores"] = per_row * n / (out["join_wall_s"] + out["resolution_wall_s"])
    dupf.close()
    pairs.close()
    s.close()
    vecs.close()
    del rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="1e6:0,1e7:2097152")
    ap.add_argument("--dup", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_duplicate_probe.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "d": D, "mode": "MSE_MODE_MFMA", "measured": "one run", "runs": []}
    for spec in a.runs.split(","):
        n, w = spec.split(":")
        res["runs"].append(one_run(int(float(n)), int(float(w)), a.dup, a.threshold, a.sample))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
