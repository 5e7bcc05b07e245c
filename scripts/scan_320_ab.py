#!/usr/bin/env python3
"""A/B of the 320-query pass of the brute-force scan at the metric's size, both arms in ONE process on one device: the one-dimensional
wave split (scan_mfma_kernel<2,20>, MSE_SCAN_2D=0) against the two-dimensional one (scan_mfma2d_kernel<2,16,0,320>, MSE_SCAN_2D unset),
alternated round by round.  Needs the developer library (make -C meme-search-engine_amd/csrc dev), which reads the knob at every launch.
Per round: scan kernel time by HIP events (scan_timing), step time, queries/s, sclk and socket power (read, never set).
  python scripts/scan_320_ab.py [rows] [seconds per round] [rounds] [extra MSE_SCAN_2D values: 164, 165 = other piece orders]   -> stdout"""
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MSE_HIP_LIB", os.path.join(ROOT, "meme-search-engine_amd", "lib", "libmse_hip_dev.so"))
os.environ.pop("MSE_SCAN_2D", None)
for p in (ROOT, os.path.join(ROOT, "meme-search-engine_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mse  # noqa: E402

D, NQ, K = 1152, 320, 10
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
secs = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
ARMS = [("1-D <2,20> (parent)", "0"), ("2-D 64x160", None)] + [(f"MSE_SCAN_2D={v}", v) for v in sys.argv[4:]]


def sample():   # as scripts/scan_pass_probe.py: reads the engine clock and socket power, sets nothing
    try:
        out = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=5).stdout
        card = next(iter(json.loads(out).values()))
        pw = next((float(v) for k, v in card.items() if "Power" in k and "W" in k), None)
        ck = next((v for k, v in card.items() if k.startswith("sclk")), None)
        mhz = int("".join(ch for ch in str(ck).split("Mhz")[0].split("(")[-1] if ch.isdigit())) if ck else None
        return mhz, pw
    except Exception:  # noqa: BLE001
        return None, None


def set_arm(v):
    if v is None:
        os.environ.pop("MSE_SCAN_2D", None)
    else:
        os.environ["MSE_SCAN_2D"] = v


vecs = mse.VectorList.generate(0x5EED0001, 0, rows, D)
s = mse.Searcher(vecs)
qs = mse.VectorList.generate(0x5EED0002, 0, 4 * NQ, D)
out_s = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
out_i = torch.empty((NQ, K), dtype=torch.int32, device="cuda")


def step(n):
    s.bruteforce_topk_dev(qs.device_ptr + (n % 4) * NQ * D * 2, NQ, K, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)


print(f"# scripts/scan_320_ab.py {rows} {secs} {rounds}: one MI355X, one process, {rows} x {D} fp16 rows, top-{K}, {NQ} queries per pass, arms alternated;")
print(f"# {torch.cuda.get_device_name(0)}; library {os.path.basename(os.environ['MSE_HIP_LIB'])}; sclk / socket power by rocm-smi every 0.5 s")
# the arms give the same answers (first step of each) before anything is timed
answers = []
for name, v in ARMS:
    set_arm(v)
    step(0)
    torch.cuda.synchronize()
    answers.append((out_s.cpu().numpy().copy(), out_i.cpu().numpy().copy(), s.last_stats()["widened_queries"]))
same = all(np.array_equal(a[0], answers[0][0]) and np.array_equal(a[1], answers[0][1]) for a in answers)
print(f"# answers of all arms equal: {same}; widened queries per arm: {[a[2] for a in answers]}")
if not same:
    sys.exit("arms disagree: nothing timed")
t0, n = time.perf_counter(), 0
while time.perf_counter() - t0 < 2.0:   # warm-up, both arms
    set_arm(ARMS[n % len(ARMS)][1])
    step(n)
    n += 1
torch.cuda.synchronize()

res = {name: [] for name, _ in ARMS}
for r in range(rounds):
    for name, v in ARMS:
        set_arm(v)
        stop, samples = threading.Event(), []

        def watch():
            while not stop.is_set():
                samples.append(sample())
                time.sleep(0.5)

        th = threading.Thread(target=watch)
        th.start()
        s.scan_timing(2)
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < secs:
            step(n)
            n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stop.set()
        th.join()
        ms, launches = s.scan_timing(0)
        good = [x for x in samples[1:] if x[0]]
        clk = sum(x[0] for x in good) / len(good) if good else float("nan")
        pws = [x[1] for x in good if x[1]]
        pw = sum(pws) / len(pws) if pws else float("nan")
        rec = (NQ * n / dt, dt / n * 1e3, ms / max(launches, 1))
        res[name].append(rec)
        print(f"round {r} {name:26s}: {rec[0]:8.1f} queries/s, step {rec[1]:7.3f} ms, scan kernel {rec[2]:7.3f} ms; sclk {clk:5.0f} MHz, socket {pw:5.0f} W", flush=True)

med = {name: statistics.median(x[0] for x in v) for name, v in res.items()}
for name, v in res.items():
    qps = [x[0] for x in v]
    print(f"{name:26s}: median {med[name]:8.1f} queries/s (min {min(qps):.1f}, max {max(qps):.1f}, spread {max(qps) - min(qps):.1f}), "
          f"median scan kernel {statistics.median(x[2] for x in v):.3f} ms, median step {statistics.median(x[1] for x in v):.3f} ms")
parent, new = ARMS[0][0], ARMS[1][0]
spread = max(x[0] for x in res[parent]) - min(x[0] for x in res[parent])
gain = med[new] - med[parent]
print(f"verdict: 2-D median - parent median = {gain:+.1f} queries/s ({gain / med[parent] * 100:+.2f} %); twice the parent arm's spread = {2 * spread:.1f}; "
      f"the 2-D form {'SHIPS' if gain > 2 * spread else 'does NOT ship'}")
