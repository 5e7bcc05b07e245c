"""Developer probe (needs a GPU), not a test: the sparse-autoencoder encode on the device (mse.SparseAutoencoder, csrc/sae.hip) over resident
rows of the hard set of bench_ann, with checkpoint-shaped random weights (down = up^T, as sae/model.py:22 of the reference starts).
  1. encode of --rows rows at (1152, 18 432, 128) next to ScoreModel.score_rows on the same rows and shape in the same run: kernel
     milliseconds (mse_sae_timing / mse_describe_timing), TFLOP/s of the up projection, and the ratio of the two -- the figure of merit, since
     the score kernel is the same tile with another epilogue
  2. one encode of --big-rows rows at the reference's size (1152, 262 144, 128), the merge and the reconstruction timed apart
  3. one single-row call at that size, automatic hidden parts against one part
Writes profiles/sae_probe.json.

python scripts/sae_probe.py [--rows N] [--big-rows N] [--big-hidden H] [--out PATH]"""
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
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--big-rows", type=int, default=10_000)
ap.add_argument("--hidden", type=int, default=18432)
ap.add_argument("--big-hidden", type=int, default=262144)
ap.add_argument("--top-k", type=int, default=128)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sae_probe.json"))
a = ap.parse_args()

n, D, K = a.rows, ba.D, a.top_k
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
rng = np.random.default_rng(7)
res = {"rows": n, "d_emb": D, "top_k": K, "runs": "one run"}


def sae_timing(enable):
    e, m = C.c_double(), C.c_double()
    ffi.check(ffi.lib().mse_sae_timing(enable, C.byref(e), C.byref(m)), "sae_timing")
    return e.value, m.value


def describe_timing(enable):
    mlp, passes = C.c_double(), (C.c_double * 3)()
    ffi.check(ffi.lib().mse_describe_timing(enable, C.byref(mlp), passes), "describe_timing")
    return mlp.value


def weights(hidden):
    up = rng.standard_normal((hidden, D), dtype=np.float32) / np.float32(np.sqrt(D))
    return up, np.ascontiguousarray(up.T)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


# 1. the encode next to the score kernel
H = a.hidden
up, down = weights(H)
sae = mse.SparseAutoencoder(up, down, top_k=K)
sm = mse.ScoreModel(up, np.zeros(H, np.float32), (rng.standard_normal((3, H)) * np.sqrt(H) / D).astype(np.float32))
sae.encode_rows(vecs, n=min(n, 4096), count=False).close()     # warm-up: the first launch loads the code object
sm.score_rows(vecs, first=0, n=min(n, 4096)).close()
sae_timing(2)
describe_timing(2)
feats, enc_wall = wall(lambda: sae.encode_rows(vecs))
scores, _ = wall(lambda: sm.score_rows(vecs))
enc_ms, mrg_ms = sae_timing(1)
mlp_ms = describe_timing(0)
flop = 2.0 * n * H * D
one = {"d_hidden": H, "encode_kernel_ms": enc_ms, "merge_kernel_ms": mrg_ms, "encode_call_wall_ms": enc_wall, "score_kernel_ms": mlp_ms,
       "encode_tflops": flop / (enc_ms * 1e-3) / 1e12 if enc_ms > 0 else None,
       "score_tflops": 2.0 * n * H * (D + 3) / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else None,
       "mean_features_per_row": float(feats.counts.astype(np.float64).mean()), "invalid_rows": feats.invalid_rows}
one["encode_over_score_tflops"] = one["encode_tflops"] / one["score_tflops"] if enc_ms > 0 and mlp_ms > 0 else None
res["encode_next_to_score"] = one
feats.close()
scores.close()
sae.close()
sm.close()
del up, down

# 2. the reference's size
H, nb = a.big_hidden, min(a.big_rows, n)
up, down = weights(H)
big, load_ms = wall(lambda: mse.SparseAutoencoder(up, down, top_k=K))
del up, down
big.encode_rows(vecs, n=min(nb, 256), count=False).close()
sae_timing(2)
feats, enc_wall = wall(lambda: big.encode_rows(vecs, n=nb))
enc_ms, mrg_ms = sae_timing(1)
feats.sq_errors()[:1]                                           # warm-up of the reconstruction kernel
sq, rec_ms = wall(lambda: feats.sq_errors())
flop = 2.0 * nb * H * D
res["reference_size"] = {"d_hidden": H, "rows": nb, "load_and_transpose_wall_ms": load_ms, "encode_kernel_ms": enc_ms, "merge_kernel_ms": mrg_ms,
                         "encode_call_wall_ms": enc_wall, "sq_errors_call_wall_ms": rec_ms,
                         "encode_tflops": flop / (enc_ms * 1e-3) / 1e12 if enc_ms > 0 else None,
                         "encode_ms_per_thousand_rows": enc_ms / nb * 1e3, "ms_per_thousand_rows_at_125_tflops": 2.0 * 1e3 * H * D / 125e12 * 1e3,
                         "mean_features_per_row": float(feats.counts.astype(np.float64).mean()), "mse": feats.mse()}
feats.close()

# 3. one row: automatic parts against one part
single = {}
for name, parts in (("automatic_parts", 0), ("one_part", 1)):
    big.set_hidden_parts(parts)
    big.encode_rows(vecs, ids=[5], count=False).close()
    sae_timing(2)
    f1, w = wall(lambda: big.encode_rows(vecs, ids=[5], count=False))
    e, m = sae_timing(1)
    single[name] = {"encode_kernel_ms": e, "merge_kernel_ms": m, "call_wall_ms": w, "features": int(f1.counts[0])}
    f1.close()
sae_timing(0)
res["single_row"] = single

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
