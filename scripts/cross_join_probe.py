"""The cross join, measured.  Not part of bench.py, not a test.

  python3 scripts/cross_join_probe.py [--rows 1e7] [--batches 128,4096,65536] [--dup 0.02] [--threshold 0.95] [--sample 16]

On one MI355X: the hard set of bench_ann.py (no micro-clusters) as the resident base, and per batch size m an incoming batch of the same
distribution in which `dup` of the rows are noisy copies of resident rows and `dup` are noisy copies of earlier rows of the batch.  Per m:
the wall time of near_duplicates_of and the HIP-event time of its phases (mse_join_timing), the tile kernel's TFLOP/s (2 x 128 x 128 x
1152 flop per tile that did work) next to the self-join's rate over the first 1e6 resident rows in the same run, pairs nominated against
pairs kept, the self-join of the batch, the time of admit and its rounds, and what the parent commit offers for the same decision: one
RowFilter.from_scores call per incoming row (timed on `sample` rows and scaled), and bruteforce_topk(k=1) of the batch plus a threshold
compare -- a faster, tuned scan that yields the best partner only.
Writes profiles/cross_join_probe.json and prints it."""
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


def incoming_batch(hs, rows, m, dup, seed):
    """[m, 1152] f16 device tensor: fresh rows of the hard set; `dup` of them overwritten by near-copies of resident rows, then `dup` by
    near-copies of earlier batch rows"""
    q = hs.rows(m, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    k = max(1, int(m * dup))
    perm = torch.randperm(m - 1, device="cuda", generator=g) + 1           # row 0 stays fresh
    from_base, from_batch = perm[:k], perm[k:2 * k]
    src = torch.randint(0, rows.shape[0], (k,), device="cuda", generator=g)

    def near(x):
        x = x.float() + torch.randn(x.shape[0], D, device="cuda", generator=g) * (0.1 / D ** 0.5)
        return (x / x.norm(dim=1, keepdim=True)).half()
    q[from_base] = near(rows[src])
    earlier = (torch.rand(k, device="cuda", generator=g) * from_batch.float()).long()
    earlier = torch.minimum(earlier, from_batch - 1)
    q[from_batch] = near(q[earlier])
    torch.cuda.synchronize()
    return q, k


def tile_rate(st, tm):
    flop = st["tiles"] * 2.0 * TILE * TILE * D
    return flop / (tm["tile_ms"] * 1e-3) / 1e12 if tm["tile_ms"] > 0 else None


def self_rate(rows, n_self, thr):
    """TFLOP/s of the self-join's tile kernel over the first n_self resident rows"""
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n_self, D, keepalive=rows)
    s = mse.Searcher(vecs)
    s.join_timing(1)
    p = s.near_duplicates(thr, mode=mse.MODE_MFMA)
    tm, st = s.join_timing(0), s.join_stats()
    p.close()
    s.close()
    vecs.close()
    return tile_rate(st, tm)


def one_batch(hs, rows, s, m, dup, thr, sample, self_tflops):
    q, planted = incoming_batch(hs, rows, m, dup, 900 + m)
    qv = mse.VectorList.wrap_device(q.data_ptr(), m, D, keepalive=q)
    out = {"incoming_rows": m, "planted_from_base": planted, "planted_from_batch": planted}
    s.join_timing(1)
    t0 = time.perf_counter()
    cross = s.near_duplicates_of(qv, thr, mode=mse.MODE_MFMA)
    out["cross_wall_s"] = time.perf_counter() - t0
    tm, st = s.join_timing(0), s.join_stats()
    tflops = tile_rate(st, tm)
    out.update({"tile_kernel_s": tm["tile_ms"] / 1e3, "rescore_s": tm["rescore_ms"] / 1e3, "list_build_s": tm["list_ms"] / 1e3, "tiles": st["tiles"],
                "tile_TFLOPs": tflops, "tile_of_f16_mfma_peak": tflops / MFMA_PEAK_TFLOPS if tflops else None,
                "self_join_tile_TFLOPs_1e6_rows": self_tflops, "tile_of_self_join_rate": tflops / self_tflops if tflops and self_tflops else None,
                "pairs_nominated": st["nominated"], "pairs_kept": st["kept"], "strips_repeated": st["strips_repeated"]})
    qs = mse.Searcher(qv)
    t0 = time.perf_counter()
    among = qs.near_duplicates(thr, mode=mse.MODE_MFMA)
    out["batch_self_join_wall_s"] = time.perf_counter() - t0
    out["batch_pairs"] = among.count
    t0 = time.perf_counter()
    adm = cross.admit(among)
    out["admit_wall_s"] = time.perf_counter() - t0
    out["admit_rounds"] = s.join_stats()["rounds"]
    out["rows_kept"] = adm.kept.count
    out["rows_dropped_by_base"] = int((adm.rep_base != mse.ID_NONE).sum())
    t0 = time.perf_counter()
    picked = qv.select(adm.kept)
    out["select_wall_s"] = time.perf_counter() - t0
    out["whole_decision_wall_s"] = out["cross_wall_s"] + out["batch_self_join_wall_s"] + out["admit_wall_s"]
    # what the parent commit offers: (a) one from_scores call per incoming row
    k = min(sample, m)
    host = q[:k].cpu().numpy().view(np.uint16)
    mse.RowFilter.from_scores(s, host[0], thr).close()
    t0 = time.perf_counter()
    for r in host:
        mse.RowFilter.from_scores(s, r, thr).close()
    per_row = (time.perf_counter() - t0) / k
    out["from_scores_per_row_s"] = per_row
    out["from_scores_all_rows_s_scaled"] = per_row * m
    out["cross_speedup_over_from_scores"] = per_row * m / out["cross_wall_s"]
    # (b) the tuned scan: the best partner only -- no complete list, no lowest-id representative, nothing about the batch itself
    hq = q.cpu().numpy().view(np.uint16)
    s.bruteforce_topk(hq[:min(m, 320)], 1, mse.MODE_MFMA)
    t0 = time.perf_counter()
    hits = 0
    for i in range(0, m, 320):                      # the scan's own batch: 320 queries per pass
        sc, _ = s.bruteforce_topk(hq[i:i + 320], 1, mse.MODE_MFMA)
        hits += int((sc[:, 0] >= thr).sum())
    out["topk1_wall_s"] = time.perf_counter() - t0
    out["topk1_rows_with_a_partner"] = hits
    out["cross_over_topk1_wall"] = out["cross_wall_s"] / out["topk1_wall_s"]
    for h in (picked, adm, among, qs, cross, qv):
        h.close()
    del q
    torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e7")
    ap.add_argument("--batches", default="128,4096,65536")
    ap.add_argument("--dup", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.95)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_join_probe.json"))
    a = ap.parse_args()
    n = int(float(a.rows))
    thr = mse.scale_dot_result(a.threshold)
    hs = bench_ann.HardSet(n, **bench_ann.HARD_PARAMS)
    rows = hs.rows(n, 5)
    torch.cuda.synchronize()
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
    s = mse.Searcher(vecs)
    res = {"device": torch.cuda.get_device_name(0), "d": D, "mode": "MSE_MODE_MFMA", "measured": "one run", "resident_rows": n,
           "threshold": a.threshold, "runs": []}
    self_tflops = self_rate(rows, min(n, 1000000), thr)
    for m in (int(x) for x in a.batches.split(",")):
        res["runs"].append(one_batch(hs, rows, s, m, a.dup, thr, a.sample, self_tflops))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
