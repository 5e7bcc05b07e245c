"""Insert into freed slots against a rebuild, on the hard synthetic set of bench_ann.py (not bench.py; nothing imports this).

For each fraction: that share of the rows is deleted (delete_rows) and as many fresh vectors are inserted back into the freed slots
(insert_rows, rows resident on the device).  Reported: inserts per second at batch 1, 64 and 1024 (each over its own share of the
slots; the shares of batch 1 and 64 are capped so that the run stays short), the time of a one-row insert, the time of a one-pass
rebuild over the same final rows by BuildGraph.build (mse_build_graph, the path that existed before the insert), and held-out
recall@10 / queries per second at search list 200 of the inserted graph against that rebuild.
Writes profiles/graph_insert_probe.json.  Needs one MI355X.

    python scripts/graph_insert_probe.py [--rows 10000000] [--fractions 0.01,0.1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "meme-search-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--fractions", default="0.01,0.1")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--search-list", type=int, default=200)
    ap.add_argument("--cap-batch-1", type=int, default=2000, help="most rows inserted at batch 1")
    ap.add_argument("--cap-batch-64", type=int, default=20000, help="most rows inserted at batch 64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_insert_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mse
    from mse import ffi
    from bench_ann import D, HARD_PARAMS, HardSet, recall_at
    n, nq, L, K, R, BATCH = a.rows, a.queries, a.search_list, 10, 64, 16384
    cfg = mse.IndexBuildConfig(r=R, l=192, maxc=750)
    hs = HardSet(n, **HARD_PARAMS)
    rows = hs.rows(n, 1)
    original = rows.clone()                                         # every fraction starts from the rows the first graph was built over
    held = hs.rows(nq, 3)
    q16 = held.cpu().numpy().view(np.uint16)
    torch.cuda.synchronize()
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
    s = mse.Searcher(vecs)
    med = mse.medioid(vecs)

    def build(seed):
        t0 = time.perf_counter()
        g = mse.BuildGraph(n, R)
        g.random_fill(seed)
        g.build(s, np.random.default_rng(seed).permutation(n).astype(np.uint32), mse.medioid(vecs), cfg, BATCH)
        return g, time.perf_counter() - t0

    g0, t_build = build(1)
    h0 = g0.to_host()
    g0.close()
    out = {"set": "hard", "rows": n, "queries": nq, "search_list": L, "beamwidth": 4, "k": K, "build": {"r": R, "l": 192, "maxc": 750, "passes": 1,
           "batch": BATCH, "seconds": t_build}, "fractions": []}

    def timed(run):
        run()
        t0 = time.perf_counter()
        top = run()
        return top, nq / (time.perf_counter() - t0)

    for fi, frac in enumerate(float(x) for x in a.fractions.split(",")):
        rng = np.random.default_rng(int(frac * 1000) + 11)
        dead = rng.random(n) < frac
        dead[med] = False
        slots = rng.permutation(np.flatnonzero(dead)).astype(np.uint32)
        m = len(slots)
        entries = np.sort(rng.choice(np.flatnonzero(~dead), max(4096, n // 1500), replace=False)).astype(np.uint32)
        fresh = hs.rows(m, 5 + fi)                                  # new vectors of the same distribution, on the device
        torch.cuda.synchronize()
        g = mse.BuildGraph(n, R, h0)
        mse.set_entries(g, vecs, entries)
        t0 = time.perf_counter()
        st = g.delete_rows(s, slots, cfg)
        row = {"fraction": frac, "rows": m, "delete_rows": dict(st, seconds=time.perf_counter() - t0), "insert_rows": {}}
        # one-row inserts first (the scratch is allocated by the first of them, which is not timed)
        one = []
        for i in range(min(9, m)):
            t0 = time.perf_counter()
            g.insert_rows(s, slots[i:i + 1], fresh[i:i + 1], cfg, med, batch=1)
            one.append(time.perf_counter() - t0)
        done = len(one)
        row["one_row_insert_ms"] = {"first_call": one[0] * 1e3, "median_of_the_rest": float(np.median(one[1:])) * 1e3 if len(one) > 1 else None}
        shares = {1: min(a.cap_batch_1, (m - done) // 3), 64: min(a.cap_batch_64, (m - done) // 3)}
        shares[1024] = m - done - shares[1] - shares[64]
        for batch in (1, 64, 1024):
            k = shares[batch]
            if k <= 0:
                continue
            t0 = time.perf_counter()
            st = g.insert_rows(s, slots[done:done + k], fresh[done:done + k], cfg, med, batch=batch)
            dt = time.perf_counter() - t0
            row["insert_rows"][f"batch_{batch}"] = dict(st, seconds=dt, inserts_per_s=k / dt)
            done += k
        assert done == m and not g.deleted().any()
        _, truth = s.bruteforce_topk(q16, K)                         # over the final rows
        top, qps = timed(lambda: mse.disk_query_topk(s, None, None, g, q16, K, None, None, None, True, 4, L)[0])
        row["inserted"] = {"recall_at_10": recall_at(top, truth), "queries_per_s": qps}
        g.close()
        g2, t_re = build(2)                                          # mse_build_graph over the same final rows
        mse.set_entries(g2, vecs, entries)
        top, qps = timed(lambda: mse.disk_query_topk(s, None, None, g2, q16, K, None, None, None, True, 4, L)[0])
        row["rebuild_seconds"] = t_re
        row["rebuilt"] = {"recall_at_10": recall_at(top, truth), "queries_per_s": qps}
        g2.close()
        out["fractions"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:          # after every fraction: a run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
        rows.copy_(original)
        torch.cuda.synchronize()
        ffi.check(ffi.lib().mse_base_rows_changed(vecs._h))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
