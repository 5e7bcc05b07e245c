"""Developer probe (needs a GPU), not a test: the device codec trainer (mse.CodecTrainer, csrc/pq_train.hip) on the hard set of bench_ann at
1e6 sample rows and 1e5 queries -- time per refine step split by mse_pq_trainer_timing, the residual GEMM's TFLOP/s against the f32-input
MFMA peak, whole-training time against bench_ann.train_codec_aopq on the same device, rows, rounds, steps and lr, and PQ-only recall@10 /
the share of the exact top-10 inside the ADC top-200 with both codecs, as scripts/codec_train_probe.py measures them.
Writes profiles/codec_train_device_probe.json.

python scripts/codec_train_device_probe.py [--rows N] [--queries M] [--rounds R] [--steps S] [--lr LR] [--skip-torch] [--skip-recall]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mse  # noqa: E402
import bench_ann as ba  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--queries", type=int, default=100_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--lr", type=float, default=5e-4)
ap.add_argument("--kmeans-iters", type=int, default=3)
ap.add_argument("--skip-torch", action="store_true")
ap.add_argument("--skip-recall", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_train_device_probe.json"))
a = ap.parse_args()

n, D = a.rows, ba.D
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
train_q = hs.rows(a.queries, 7).float()
res = {"rows": n, "queries": a.queries, "rounds": a.rounds, "steps": a.steps, "lr": a.lr, "kmeans_iters": a.kmeans_iters}

# ---- the device trainer: the sample is the resident rows themselves, gathered on the device -----------------------------------
t0 = time.perf_counter()
tr = mse.CodecTrainer()
tr.set_sample_rows(vecs, np.arange(n, dtype=np.uint32))
tr.init(4)
tr.set_queries(train_q.cpu().numpy())
res["setup_s"] = time.perf_counter() - t0
t1 = time.perf_counter()
res["empty_cells_after_kmeans"] = tr.kmeans(a.kmeans_iters)
res["kmeans_s"] = time.perf_counter() - t1
hist, refine_s, rotation_s = [], 0.0, 0.0
for _ in range(a.rounds):
    t1 = time.perf_counter()
    losses = tr.refine(a.steps, lr=a.lr)
    refine_s += time.perf_counter() - t1
    hist += [losses[0], losses[-1]]
    t1 = time.perf_counter()
    tr.update_rotation()
    rotation_s += time.perf_counter() - t1
res["device_training_s"] = time.perf_counter() - t0
res["refine_s"], res["rotation_update_s"] = refine_s, rotation_s
res["refine_step_ms"] = 1e3 * refine_s / max(a.rounds * a.steps, 1)
res["last_step_ms"] = tr.timing()
res["query_aware_loss_first_last_per_round"] = hist
props = torch.cuda.get_device_properties(0)
clock_khz = getattr(props, "clock_rate", None)      # not every torch build reports it: then the part's nominal 2.4 GHz
clock_hz = clock_khz * 1e3 if clock_khz else 2.4e9
res["clock_ghz"], res["clock_source"] = clock_hz / 1e9, "device properties" if clock_khz else "nominal (the clock under load was not measured)"
flop = 2.0 * n * D * D
res["gemm_tflops"] = flop / (res["last_step_ms"]["gemm"] * 1e-3) / 1e12 if res["last_step_ms"]["gemm"] > 0 else None
res["f32_mfma_peak_tflops"] = 64 * 4 * props.multi_processor_count * clock_hz / 1e12      # 64 FLOP / clk / SIMD at clock_ghz
res["untuned_f32_mfma_gemm_tflops_4096_cubed"] = 122.0
cents, T = tr.arrays()
tr.close()
print(json.dumps(res), flush=True)

codecs = {"device": (cents, T)}
if not a.skip_torch:
    t0 = time.perf_counter()
    c2, T2, info = ba.train_codec_aopq(rows.float(), train_q, rounds=a.rounds, iters=a.steps, lr=a.lr, kmeans_iters=a.kmeans_iters)
    torch.cuda.synchronize()
    res["torch_training_s"] = time.perf_counter() - t0
    res["torch_loss_first_last_per_round"] = info["query_aware_loss_first_last_per_round"]
    codecs["torch"] = (c2, T2)

if not a.skip_recall:
    s = mse.Searcher(vecs)
    q = hs.rows(1024, 2)
    q32 = q.float().cpu().numpy()
    _, truth = s.bruteforce_topk(q.cpu().numpy().view(np.uint16), 10)
    for name, (c, t) in codecs.items():
        pq = mse.ProductQuantizer(c, t, 18, D)
        codes = mse.Codes.quantize_base(pq, vecs)
        top10 = np.concatenate([pq.scan_topk_batch(codes, q32[i:i + 64], 10, 10, None)[1] for i in range(0, 1024, 64)])
        top200 = np.concatenate([pq.scan_topk_batch(codes, q32[i:i + 64], 200, 200, None)[1] for i in range(0, 1024, 64)])
        res[name + "_pq_only_recall_at_10"] = float(ba.recall_at(top10, truth))
        res[name + "_exact_top10_inside_adc_top200"] = sum(len(set(top200[i].tolist()) & set(truth[i].tolist())) for i in range(1024)) / 10240

os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
