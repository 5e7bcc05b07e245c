"""Developer probe (needs a GPU), not a test: sparse-autoencoder training on the device (mse.SaeTrainer, csrc/sae_train.hip) over resident
rows of the hard set of bench_ann, from SparseAutoencoder.random weights, batch 64, at (1152, 18 432, 128) and at the reference's
(1152, 262 144, 128) (sae/train.py:25-39).  Per size:
  1. milliseconds per step and per stage (mse_sae_trainer_timing: forward with the gate, the small backward kernels, the dense update),
     with the touched-row skip off -- the dense pass then moves 12 arrays of d_hidden x d_emb floats -- and with it on
  2. the dense pass's bytes over its time as a share of the device's copy rate, which the script measures itself in the same run (a
     device-to-device copy of one such array by torch's vectorised copy kernel, read + write bytes, median of seven)
  3. the same step written with torch on the same device -- this script's own eager restatement of sae/model.py:31-43 and
     sae/train.py:51-59 with torch.optim.AdamW, fp32 matmuls -- timed alternately with ours, medians of wall time with a device
     synchronisation around each step
  4. RowFeatures.mse() of held-out rows before and after --train-steps steps
Writes profiles/sae_train_probe.json.

python scripts/sae_train_probe.py [--hidden 18432,262144] [--rows N] [--train-steps N] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "meme-search-engine_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import mse  # noqa: E402
from mse import ffi  # noqa: E402
import bench_ann as ba  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", default="18432,262144")
ap.add_argument("--rows", type=int, default=40_000)
ap.add_argument("--top-k", type=int, default=128)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--timed-steps", type=int, default=10)
ap.add_argument("--train-steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sae_train_probe.json"))
a = ap.parse_args()

n, D, K, B = a.rows, ba.D, a.top_k, a.batch
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
held_out = np.arange(n - 2048, n)
rng = np.random.default_rng(11)
res = {"rows": n, "d_emb": D, "top_k": K, "batch": B, "runs": "one run", "guide_copy_rate_tb_s": 6.29}


def timing(enable):
    out = (C.c_double * 4)()
    ffi.check(ffi.lib().mse_sae_trainer_timing(enable, out), "sae_trainer_timing")
    return list(out)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def copy_rate(count):
    """TB/s of a device copy of `count` floats, read + write"""
    src, dst = torch.empty(count, dtype=torch.float32, device="cuda").normal_(), torch.empty(count, dtype=torch.float32, device="cuda")
    dst.copy_(src)
    times = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return 2.0 * count * 4 / (statistics.median(times) * 1e-3) / 1e12, times


class TorchStep:
    """sae/model.py:31-43 and sae/train.py:51-59, eager"""

    def __init__(self, up, down, down_bias, lr):
        dev = "cuda"
        self.W1 = torch.tensor(up, device=dev, requires_grad=True)
        self.W2 = torch.tensor(down, device=dev, requires_grad=True)
        self.b2 = torch.tensor(down_bias, device=dev, requires_grad=True)
        self.opt = torch.optim.AdamW([self.W1, self.W2, self.b2], lr=lr, weight_decay=0.0)

    def step(self, x):
        self.opt.zero_grad()
        h = F.relu(F.linear(x, self.W1))
        thr = torch.kthvalue(h, k=h.shape[-1] - K, dim=-1).values.unsqueeze(-1).expand_as(h)
        h = torch.where(h > thr, h, torch.zeros_like(h))
        loss = F.mse_loss(F.linear(h, self.W2, self.b2), x)
        loss.backward()
        self.opt.step()
        return loss


def batch_ids(steps):
    return rng.integers(0, n - 2048, steps * B).astype(np.uint32)


for H in [int(h) for h in a.hidden.split(",")]:
    one = {"d_hidden": H}
    sae = mse.SparseAutoencoder.random(D, H, K, seed=5)
    up, down, _, down_bias = sae.weights()
    tr = mse.SaeTrainer(sae, lr=3e-4)
    one["held_out_mse_before"] = sae.encode_rows(vecs, ids=held_out, count=False).mse()
    tr.train(vecs, batch_ids(2), B)                              # warm-up: the first launches load the code object
    one["copy_rate_tb_s"], one["copy_ms_each"] = copy_rate(H * D)
    array_bytes = H * D * 4.0
    for name, skip in (("all_rows", False), ("touched_rows_only", True)):
        tr.set_skip(skip)
        timing(2)
        losses, ms = wall(lambda: tr.train(vecs, batch_ids(a.timed_steps), B))
        fwd, bwd, upd, steps = timing(0)
        touched = int((sae.counters() > 0).sum())
        st = {"steps": int(steps), "call_wall_ms_per_step": ms / a.timed_steps, "forward_ms_per_step": fwd / steps, "backward_ms_per_step": bwd / steps,
              "update_ms_per_step": upd / steps, "features_that_have_fired": touched}
        moved = 12 * array_bytes if not skip else 12 * array_bytes * touched / H
        st["update_bytes_per_step"] = moved
        st["update_tb_s"] = moved / (upd / steps * 1e-3) / 1e12
        st["update_share_of_copy_rate"] = st["update_tb_s"] / one["copy_rate_tb_s"]
        one[name] = st
    # the torch step beside ours, alternately
    tstep = TorchStep(up, down, down_bias, 3e-4)
    x_all = rows                                                 # [n, 1152] f16 on the device
    tstep.step(x_all[torch.from_numpy(batch_ids(1).astype(np.int64)).cuda()].float())
    ours, theirs = [], []
    for _ in range(a.rounds):
        ids = batch_ids(1)
        _, ms = wall(lambda: tr.step(vecs, ids))
        ours.append(ms)
        x = x_all[torch.from_numpy(ids.astype(np.int64)).cuda()].float()
        _, ms = wall(lambda: tstep.step(x))
        theirs.append(ms)
    one["step_wall_ms_ours"], one["step_wall_ms_torch"] = statistics.median(ours), statistics.median(theirs)
    one["step_wall_ms_ours_each"], one["step_wall_ms_torch_each"] = ours, theirs
    one["torch_over_ours"] = one["step_wall_ms_torch"] / one["step_wall_ms_ours"]
    del tstep
    torch.cuda.empty_cache()
    # the held-out error after a fixed number of further steps
    losses = tr.train(vecs, batch_ids(a.train_steps), B)
    one["train_steps_total"] = tr.steps
    one["loss_first_of_last_call"], one["loss_last"] = float(losses[0]), float(losses[-1])
    one["held_out_mse_after"] = sae.encode_rows(vecs, ids=held_out, count=False).mse()
    res["d_hidden_%d" % H] = one
    print(json.dumps(one), flush=True)
    tr.close()
    sae.close()
    del up, down

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
