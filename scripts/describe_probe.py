"""Developer probe (needs a GPU), not a test: descriptors on the device (mse.ScoreModel.score_rows, mse.RowScores, mse.Codes.describe;
csrc/describe.hip) at the shipped model shape (1152, 18 432, 3) over resident rows of the hard set of bench_ann.  Reports the fused MLP's
kernel time (mse_describe_timing) and TFLOP/s against the f32-MFMA peak (--peak-tflops, default 157.3 = 256 CUs x 4 SIMDs x 64 FLOP/clk x
2.4 GHz) and against the 122 TFLOP/s of an untuned LDS-tiled f32-MFMA GEMM; the select's three counting passes in GB/s of keys read
(useful bytes: 4 per key; the column is strided, so the lines touched are channels x that) against the copy rate (--copy-gbps); the wall
time of the whole describe (scores, CDF fit, descriptor bytes); and the existing host-in / host-out score_batch on 2 048 of the same rows,
scaled to all rows, as the thing replaced.  Writes profiles/describe_probe.json.

python scripts/describe_probe.py [--rows N] [--copy-gbps R] [--peak-tflops P]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mse  # noqa: E402
from mse import ffi  # noqa: E402
import bench_ann as ba  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--hidden", type=int, default=18432)
ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--copy-gbps", type=float, default=None, help="the device copy rate scripts/microbench measured, for the ratio")
ap.add_argument("--peak-tflops", type=float, default=157.3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_probe.json"))
a = ap.parse_args()

NOT = "not measured yet"
n, D, H, CH = a.rows, ba.D, a.hidden, a.channels
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
rng = np.random.default_rng(7)
up = (rng.standard_normal((H, D)) / np.sqrt(D)).astype(np.float32)
bias = rng.standard_normal(H).astype(np.float32)
down = (rng.standard_normal((CH, H)) * np.sqrt(H) / D).astype(np.float32)
sm = mse.ScoreModel(up, bias, down)
ts = rng.integers(1_500_000_000, 1_760_000_000, n).astype(np.int64)
res = {"rows": n, "shape": [D, H, CH]}


def timing(enable):
    mlp, passes = C.c_double(), (C.c_double * 3)()
    ffi.check(ffi.lib().mse_describe_timing(enable, C.byref(mlp), passes), "describe_timing")
    return mlp.value, [float(p) for p in passes]


sm.score_rows(vecs, first=0, n=min(n, 4096)).close()            # warm-up: the first launch loads the code object
timing(2)
torch.cuda.synchronize()
t0 = time.perf_counter()
scores = sm.score_rows(vecs, timestamps=ts)
t_scores = time.perf_counter() - t0
mlp_ms, _ = timing(1)
flop = 2.0 * n * H * (D + CH)
res["mlp_kernel_ms"] = mlp_ms
res["mlp_tflops"] = flop / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else None
res["mlp_over_f32_mfma_peak"] = res["mlp_tflops"] / a.peak_tflops if mlp_ms > 0 else None
res["mlp_over_untuned_gemm_122_tflops"] = res["mlp_tflops"] / 122.0 if mlp_ms > 0 else None

t0 = time.perf_counter()
cdfs = scores.fit_cdfs()
t_fit = time.perf_counter() - t0
_, pass_ms = timing(0)                                           # of the last select: the timestamp channel, unit stride
res["fit_cdfs_s"] = t_fit
res["select_pass_ms_timestamps"] = pass_ms
res["select_pass_gbytes_per_s_timestamps"] = [n * 4 / (p * 1e-3) / 1e9 if p > 0 else None for p in pass_ms]
timing(2)
scores.order_statistics(0, np.arange(0, n, max(1, n // 510))[:510])
_, pass_ms = timing(0)
res["select_pass_ms_score_channel"] = pass_ms
res["select_pass_useful_gbytes_per_s_score_channel"] = [n * 4 / (p * 1e-3) / 1e9 if p > 0 else None for p in pass_ms]
res["copy_gbytes_per_s"] = a.copy_gbps if a.copy_gbps else NOT
res["select_pass1_over_copy_rate"] = res["select_pass_gbytes_per_s_timestamps"][0] / a.copy_gbps if a.copy_gbps and pass_ms[0] > 0 else NOT

codes = mse.Codes(np.zeros((n, 64), np.uint8), np.zeros((n, CH + 1), np.uint8))
t0 = time.perf_counter()
codes.describe(scores, cdfs)
t_desc = time.perf_counter() - t0
res["describe_bytes_s"] = t_desc
res["whole_describe_s"] = t_scores + t_fit + t_desc

m = min(n, 2048)
x = rows[:m].float().cpu().numpy()
sm.score_batch(x[:64])
t0 = time.perf_counter()
old = sm.score_batch(x)
t_old = time.perf_counter() - t0
res["score_batch_2048_rows_s"] = t_old
res["score_batch_scaled_to_all_rows_s"] = t_old * n / m
res["score_batch_over_fused"] = (t_old * n / m) / t_scores
new = scores.to_host()[0][:m]
res["largest_difference_to_score_batch"] = float(np.max(np.abs(new - old)))

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
