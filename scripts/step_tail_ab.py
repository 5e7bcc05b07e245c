#!/usr/bin/env python3
"""A/B of one whole brute-force step (mse_bruteforce_topk_f16_dev, 320 queries, MODE_MFMA) at the metric's size between BUILDS of the
library: the parent commit's libmse_hip.so against this tree's, alternated round by round, every arm of every round in a fresh child
process (MSE_HIP_LIB selects the library; the parent process never opens the device).
Per child: queries/s of whole steps over >= `seconds`, the scan kernel's HIP-event time, and step - scan = the tail.
  python scripts/step_tail_ab.py [rows] [seconds per round] [rounds] name=/path/to/lib.so name=/path/to/lib.so ...   -> stdout
An arm may carry settings after its library, separated by commas: name=/path/to/lib.so,KEY=VALUE,...
  sparse=off|auto|forced, stride=S, cap=N   the searcher's sparse-maxima knob (Searcher.set_sparse_maxima), set before the first step
  late:NAME=VALUE                           an environment variable set AFTER the first step, and every step then uses the first step's
                                            queries: a timing ablation of the developer library whose scan leaves the group maxima of
                                            that first, unablated step in place (MSE_SCAN_ABL=32), so that the tail runs as usual
The FIRST arm is the yardstick (the parent commit's build).  Rule: an arm counts as a gain if its queries/s are above the yardstick's in
every round and the difference of the means is more than twice the spread (max - min) of the yardstick's rounds."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NQ, K = 1152, 320, 10


def child(rows, secs, opts=""):
    opts = [o for o in opts.split(",") if o]
    late = dict(o[5:].split("=", 1) for o in opts if o.startswith("late:"))
    knob = dict(o.split("=", 1) for o in opts if not o.startswith("late:"))
    for p in (ROOT, os.path.join(ROOT, "meme-search-engine_amd")):
        sys.path.insert(0, p)
    import torch
    import mse
    vecs = mse.VectorList.generate(0x5EED0001, 0, rows, D)
    s = mse.Searcher(vecs)
    qs = mse.VectorList.generate(0x5EED0002, 0, 4 * NQ, D)
    out_s = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    out_i = torch.empty((NQ, K), dtype=torch.int32, device="cuda")

    if knob:
        s.set_sparse_maxima(knob.get("sparse", "auto"), int(knob.get("stride", 0)), int(knob.get("cap", 0)))

    def step(n):
        if late:
            n = 0
        s.bruteforce_topk_dev(qs.device_ptr + (n % 4) * NQ * D * 2, NQ, K, out_s.data_ptr(), out_i.data_ptr(), mse.MODE_MFMA)

    step(0)
    torch.cuda.synchronize()
    digest = hashlib.sha256(out_s.cpu().numpy().tobytes() + out_i.cpu().numpy().tobytes()).hexdigest()[:16]
    stats = s.last_stats()
    widened = stats["widened_queries"]
    os.environ.update(late)
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < 1.5:   # warm-up
        step(n)
        n += 1
    torch.cuda.synchronize()
    s.scan_timing(2)
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < secs:
        step(n)
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms, launches = s.scan_timing(0)
    print("RESULT " + json.dumps({"qps": NQ * n / dt, "step_ms": dt / n * 1e3, "scan_ms": ms / max(launches, 1), "steps": n,
                                  "answer": digest, "widened": widened,
                                  "stats": {k: v for k, v in stats.items() if k.startswith("sparse")}}), flush=True)


def main():
    if sys.argv[1] == "--child":
        return child(int(float(sys.argv[2])), float(sys.argv[3]), sys.argv[4] if len(sys.argv) > 4 else "")
    rows, secs, rounds = int(float(sys.argv[1])), float(sys.argv[2]), int(sys.argv[3])
    arms = [a.split("=", 1) for a in sys.argv[4:]]
    opts = {name: spec.partition(",")[2] for name, spec in arms}
    arms = [(name, spec.partition(",")[0]) for name, spec in arms]
    print(f"# scripts/step_tail_ab.py: one MI355X, {rows} x {D} fp16 rows, top-{K}, {NQ} queries per step, MODE_MFMA; {rounds} rounds of >= {secs} s,")
    print("# arms alternated, a fresh process per arm per round; tail = whole step - scan kernel (HIP events)")
    for name, lib in arms:
        print(f"# arm {name}: {os.path.relpath(lib, ROOT)}" + (f" with {opts[name]}" if opts[name] else ""))
    res = {name: [] for name, _ in arms}
    for r in range(rounds):
        for name, lib in arms:
            env = dict(os.environ, MSE_HIP_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(rows), str(secs), opts[name]], env=env, capture_output=True,
                               text=True, timeout=180)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:   # a child that failed ends the whole measurement: nothing more is started
                print(f"round {r} {name}: child failed with status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
                return 1
            rec = json.loads(line[7:])
            res[name].append(rec)
            print(f"round {r} {name:12s}: {rec['qps']:8.1f} queries/s, step {rec['step_ms']:7.3f} ms, scan kernel {rec['scan_ms']:7.3f} ms, "
                  f"tail {rec['step_ms'] - rec['scan_ms']:6.3f} ms, {rec['steps']} steps, widened {rec['widened']}, answer {rec['answer']}"
                  + (f", {rec['stats']}" if rec.get("stats") else ""), flush=True)
    answers = {rec["answer"] for v in res.values() for rec in v}
    print(f"answers of the first step equal in every arm and round: {len(answers) == 1}")
    base = arms[0][0]
    bq = [x["qps"] for x in res[base]]
    spread = max(bq) - min(bq)
    for name, _ in arms:
        v = res[name]
        q = [x["qps"] for x in v]
        print(f"{name:12s}: mean {statistics.mean(q):8.1f} queries/s (min {min(q):.1f}, max {max(q):.1f}, spread {max(q) - min(q):.1f}); "
              f"mean step {statistics.mean(x['step_ms'] for x in v):.3f} ms, scan kernel {statistics.mean(x['scan_ms'] for x in v):.3f} ms, "
              f"tail {statistics.mean(x['step_ms'] - x['scan_ms'] for x in v):.3f} ms")
    for name, _ in arms[1:]:
        q = [x["qps"] for x in res[name]]
        gain = statistics.mean(q) - statistics.mean(bq)
        every = all(a > b for a, b in zip(q, bq))
        print(f"verdict {name} against {base}: {gain:+.1f} queries/s ({gain / statistics.mean(bq) * 100:+.2f} %), above it in every round: {every}; "
              f"twice the spread of {base}: {2 * spread:.1f} -> {'a gain' if every and gain > 2 * spread else 'NOT a gain by the rule'}")
    return 0 if len(answers) == 1 else 1


if __name__ == "__main__":
    sys.exit(main())
