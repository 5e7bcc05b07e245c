"""Developer probe (needs a GPU), not a test: the shard partition (mse.ShardPartitioner, csrc/partition.hip) on the hard set of bench_ann --
5e5 sample rows gathered from the resident index (kmeans.py:9), S = 42, the assignment over all rows.  Reports ms per annealing iteration
and its split (mse_partition_timing), the counting pass's row bytes per second and f64 FMA rate, the same pass as a plain torch formulation
written for this probe (f32 matmul, topk, bincount) on the same device and rows, alternated, medians of 7; assignment seconds and the walk's
share (the same rows with the walk alone is not separable from outside, so the share is 1 - score-pass time / total); F after the
iterations; the shard sizes.  The recall leg (entries into a graph index at L 200 against bench_ann.shard_centroid_entries) needs a built
graph index and is reported as "not measured yet".  Writes profiles/partition_probe.json.

python scripts/partition_probe.py [--rows N] [--sample M] [--shards S] [--iters I] [--copy-gbps R]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mse  # noqa: E402
import bench_ann as ba  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--sample", type=int, default=500_000)
ap.add_argument("--shards", type=int, default=42)
ap.add_argument("--iters", type=int, default=2000)
ap.add_argument("--copy-gbps", type=float, default=None, help="the device copy rate scripts/microbench measured, for the ratio")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_probe.json"))
a = ap.parse_args()

NOT = "not measured yet"
n, D, S = a.rows, ba.D, a.shards
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
res = {"rows": n, "sample": a.sample, "shards": S, "iters": a.iters}

ids = np.random.default_rng(7).choice(n, a.sample, replace=False).astype(np.uint32)
p = mse.ShardPartitioner(S, D, seed=7)
p.set_sample(vecs, ids)
p.anneal(8)                                   # warm-up: the first launches load the code objects
torch.cuda.synchronize()
t0 = time.perf_counter()
F, code = p.anneal(a.iters)
dt = time.perf_counter() - t0
st = p.state()
res["iterations_run"] = int(len(F))
res["anneal_ms_per_iteration"] = 1e3 * dt / max(len(F), 1)
ms = p.timing()
res["last_iteration_ms"] = {"candidate_and_normalise": float(ms[0]), "count": float(ms[1]), "decide": float(ms[2])}
res["F_after"] = int(st.last_fitness)
res["F_over_n"] = float(st.last_fitness) / a.sample
res["stopped"] = int(st.stopped)
res["accepted_rejected_rerolled"] = [int((code == c).sum()) for c in (1, 0, 2)]

# ---- the counting pass alone against a plain torch formulation, alternated -------------------------------------------------------
cen = p.centroids()
x = rows[torch.from_numpy(ids.astype(np.int64)).cuda()]
x32 = x.float()
cen_t = torch.from_numpy(cen).cuda()


def torch_pass():
    sizes = torch.zeros(2, S, dtype=torch.int64, device="cuda")
    for i in range(0, x32.shape[0], 31768):                    # kmeans.py:73's batch
        idx = (x32[i:i + 31768] @ cen_t.T).topk(2, dim=1).indices
        for j in range(2):
            sizes[j] += torch.bincount(idx[:, j], minlength=S)
    return sizes


ours, theirs = [], []
for _ in range(7):
    torch.cuda.synchronize(); t0 = time.perf_counter(); sz = p.count(cen); ours.append(time.perf_counter() - t0)
    torch.cuda.synchronize(); t0 = time.perf_counter(); tz = torch_pass(); torch.cuda.synchronize(); theirs.append(time.perf_counter() - t0)
res["count_call_ms_median_of_7"] = 1e3 * statistics.median(ours)
res["torch_f32_pass_ms_median_of_7"] = 1e3 * statistics.median(theirs)
res["rows_differently_counted_by_the_f32_pass"] = int(np.abs(sz.astype(np.int64) - tz.cpu().numpy()).sum() // 2)
kernel_s = float(ms[1]) * 1e-3
res["count_kernel_row_gbytes_per_s"] = a.sample * D * 2 / kernel_s / 1e9 if kernel_s > 0 else None
res["count_kernel_f64_fma_tflops"] = 2.0 * a.sample * D * S / kernel_s / 1e12 if kernel_s > 0 else None
res["copy_gbytes_per_s"] = a.copy_gbps if a.copy_gbps else NOT
res["count_over_copy_rate"] = res["count_kernel_row_gbytes_per_s"] / a.copy_gbps if a.copy_gbps and kernel_s > 0 else NOT

# ---- the assignment over all rows ---------------------------------------------------------------------------------------------
torch.cuda.synchronize()
t0 = time.perf_counter()
p.assign(vecs, 0.2)
res["assign_s"] = time.perf_counter() - t0
score_only_s = kernel_s * n / a.sample                           # the same kernel's rate, without the score write
res["assign_walk_share"] = max(0.0, 1.0 - score_only_s / res["assign_s"])
counts = p.counts()
res["shard_sizes"] = [int(c) for c in counts]
res["shard_size_max_over_mean"] = float(counts.max() / counts.mean())

# ---- recall with these entries against the stand-in's -------------------------------------------------------------------------
res["recall_at_10_L200"] = res["queries_per_s_L200"] = res["stand_in_recall_at_10_L200"] = res["stand_in_queries_per_s_L200"] = NOT

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
