"""Developer probe (needs a GPU), not a test: the ensemble rater on the device (mse.Rater, mse.RaterTrainer, mse.MemberScores;
csrc/rater.hip) at the shipped shape (1152, 16 members, 3 channels) over resident rows of the hard set of bench_ann, from Rater.random
weights, at batch 1 and batch 64:
  1. the dense pass (mse_rater_trainer_timing): its bytes -- up and its two moment arrays, read and written, six times 85 MB -- over its
     time, against a device-to-device copy of ONE such array timed in the same run (torch's vectorised copy kernel, read + write
     bytes, median of seven).  85 MB fits the last-level cache and the pass's 0.5 GB do not, so the copy rate flatters the comparison
  2. whole-step wall time (a device synchronisation around each step) against the 0.6 GB a step must move (the pass and one read of up
     for the forward) at that copy rate, and against the same step in eager torch on the same device -- this script's restatement of
     meme-rater/model.py and train.py:63-69 with torch.optim.AdamW, fp32 -- alternately, medians of seven
  3. member scores of --rows rows next to ScoreModel.score_rows of the exported wide model on the same rows, alternately, medians of
     seven of wall time; TFLOP/s of the up projection (2 x rows x 18 432 x 1152) for both, and score_mlp_kernel's own kernel time
     (mse_describe_timing)
  4. pair_variance of 131 072 random pairs over that table, wall time, median of seven
Writes profiles/rater_probe.json.

python scripts/rater_probe.py [--rows N] [--rounds N] [--out PATH]"""
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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import mse  # noqa: E402
from mse import ffi  # noqa: E402
import bench_ann as ba  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=16384)
ap.add_argument("--members", type=int, default=16)
ap.add_argument("--channels", type=int, default=3)
ap.add_argument("--timed-steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--pairs", type=int, default=131072)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rater_probe.json"))
a = ap.parse_args()

n, D, M, Cc = a.rows, ba.D, a.members, a.channels
hs = ba.HardSet(n, **ba.HARD_PARAMS)
rows = hs.rows(n, 1)
vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
rng = np.random.default_rng(11)
array_bytes = M * D * D * 4.0
res = {"rows": n, "d_emb": D, "members": M, "channels": Cc, "runs": "one run", "array_mb": array_bytes / 1e6}


def timing(enable):
    out = (C.c_double * 4)()
    ffi.check(ffi.lib().mse_rater_trainer_timing(enable, out), "rater_trainer_timing")
    return list(out)


def describe_timing(enable):
    mlp, passes = C.c_double(), (C.c_double * 3)()
    ffi.check(ffi.lib().mse_describe_timing(enable, C.byref(mlp), passes), "describe_timing")
    return mlp.value


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


class TorchMember(nn.Module):
    def __init__(self, up, bias, down):
        super().__init__()
        self.hidden, self.output = nn.Linear(D, D), nn.Linear(D, Cc)
        with torch.no_grad():
            self.hidden.weight.copy_(torch.tensor(up))
            self.hidden.bias.copy_(torch.tensor(bias))
            self.output.weight.copy_(torch.tensor(down))
            self.output.bias.zero_()

    def forward(self, x):
        return self.output(F.silu(self.hidden(x)))


class TorchStep:
    """meme-rater/model.py:31-52 and train.py:63-69, eager"""

    def __init__(self, up, bias, down, lr):
        self.members = nn.ModuleList([TorchMember(up[m * D:(m + 1) * D], bias[m * D:(m + 1) * D], down[:, m * D:(m + 1) * D]) for m in range(M)]).cuda()
        self.opt = torch.optim.AdamW(self.members.parameters(), lr=lr, weight_decay=0.0)

    def step(self, x, y):                                      # x [M, B, 2, D], y [M, B, C]
        self.opt.zero_grad()
        s1 = torch.stack([mod(x[m, :, 0]) for m, mod in enumerate(self.members)])
        s2 = torch.stack([mod(x[m, :, 1]) for m, mod in enumerate(self.members)])
        loss = F.binary_cross_entropy(torch.sigmoid(s1 - s2), y)
        loss.backward()
        self.opt.step()
        return loss


def batch_of(steps, B):
    return rng.integers(0, n, (steps, M, B, 2)).astype(np.uint32), rng.choice([0.1, 0.3, 0.5, 0.7, 0.9], (steps, M, B, Cc)).astype(np.float32)


rater = mse.Rater.random(D, M, Cc, np.random.default_rng(5))
up, bias, down = rater.weights()
tr = mse.RaterTrainer(rater, lr=3e-4)
tr.run(vecs, *batch_of(2, 1))                                    # warm-up: the first launches load the code object
res["copy_rate_tb_s"], res["copy_ms_each"] = copy_rate(M * D * D)
tstep = TorchStep(up, bias, down, 3e-4)
for B in (1, 64):
    one = {"batch": B}
    tr.run(vecs, *batch_of(1, B))
    timing(2)
    _, ms = wall(lambda: tr.run(vecs, *batch_of(a.timed_steps, B)))
    fwd, bwd, upd, steps = timing(0)
    one.update(steps=int(steps), call_wall_ms_per_step=ms / a.timed_steps, forward_ms_per_step=fwd / steps, backward_ms_per_step=bwd / steps,
               update_ms_per_step=upd / steps)
    one["update_bytes_per_step"] = 6 * array_bytes
    one["update_tb_s"] = 6 * array_bytes / (upd / steps * 1e-3) / 1e12
    one["update_share_of_copy_rate"] = one["update_tb_s"] / res["copy_rate_tb_s"]
    one["step_floor_ms_at_copy_rate"] = 7 * array_bytes / (res["copy_rate_tb_s"] * 1e12) * 1e3
    ids, y = batch_of(1, B)
    xt = rows[torch.from_numpy(ids[0].astype(np.int64)).cuda()].float()
    tstep.step(xt, torch.tensor(y[0]).cuda())
    ours, theirs = [], []
    for _ in range(a.rounds):
        ids, y = batch_of(1, B)
        _, ms = wall(lambda: tr.run(vecs, ids, y))
        ours.append(ms)
        xt, yt = rows[torch.from_numpy(ids[0].astype(np.int64)).cuda()].float(), torch.tensor(y[0]).cuda()
        _, ms = wall(lambda: tstep.step(xt, yt))
        theirs.append(ms)
    one["step_wall_ms_ours"], one["step_wall_ms_torch"] = statistics.median(ours), statistics.median(theirs)
    one["step_wall_ms_ours_each"], one["step_wall_ms_torch_each"] = ours, theirs
    one["torch_over_ours"] = one["step_wall_ms_torch"] / one["step_wall_ms_ours"]
    one["ours_over_floor"] = one["step_wall_ms_ours"] / one["step_floor_ms_at_copy_rate"]
    res["batch_%d" % B] = one
    print(json.dumps(one), flush=True)
del tstep
torch.cuda.empty_cache()

# member scores next to the exported wide model's score kernel on the same rows
sm = rater.to_score_model()
flop = 2.0 * n * M * D * D
rater.member_scores(vecs).close()
sm.score_rows(vecs).close()
ours, theirs, kernel = [], [], []
for _ in range(a.rounds):
    t, ms = wall(lambda: rater.member_scores(vecs))
    t.close()
    ours.append(ms)
    describe_timing(2)
    t, ms = wall(lambda: sm.score_rows(vecs))
    kernel.append(describe_timing(0))
    t.close()
    theirs.append(ms)
sc = {"rows": n, "member_scores_wall_ms": statistics.median(ours), "score_rows_wall_ms": statistics.median(theirs), "score_mlp_kernel_ms": statistics.median(kernel),
      "member_scores_wall_ms_each": ours, "score_rows_wall_ms_each": theirs}
sc["member_scores_tflops"] = flop / (sc["member_scores_wall_ms"] * 1e-3) / 1e12
sc["score_rows_tflops"] = flop / (sc["score_rows_wall_ms"] * 1e-3) / 1e12
sc["score_mlp_kernel_tflops"] = flop / (sc["score_mlp_kernel_ms"] * 1e-3) / 1e12 if sc["score_mlp_kernel_ms"] else None
res["member_scores"] = sc
print(json.dumps(sc), flush=True)

table = rater.member_scores(vecs)
pa, pb = rng.integers(0, n, a.pairs), rng.integers(0, n, a.pairs)
table.pair_variance(pa, pb)
times = [wall(lambda: table.pair_variance(pa, pb))[1] for _ in range(a.rounds)]
res["pair_variance"] = {"pairs": a.pairs, "wall_ms": statistics.median(times), "wall_ms_each": times}

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
