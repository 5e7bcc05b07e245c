"""Compaction and growth of a live graph index (DeviceGraph/BuildGraph.compact) on the hard synthetic set of bench_ann.py (not bench.py;
nothing imports this).

For each deleted fraction (delete_rows first) and each capacity (the live count, and 1.25 x n):
  compact        wall time of the call; the row-gather kernel's own time (HIP events around that launch: Searcher.compact_timing) and
                 the bytes it read (n_live rows) and wrote (capacity rows) over that time, as GB/s and as a fraction of the part's
                 measured float4 copy rate (6.29 TB/s read + written)
  host trip      what the call replaces, timed in the same run: to_host, reading the rows back, a numpy renumbering, a fresh upload
  brute force    the 128-query pass over the base before and after
  graph search   held-out recall@10 and queries per second at search list 200 before and after (entry table set again through the map)
Writes profiles/graph_compact_probe.json.  Needs one MI355X with room for the old and the new index together.

    python scripts/graph_compact_probe.py [--rows 10000000] [--fractions 0.1,0.5]
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

COPY_RATE = 6.29e12   # bytes per second read + written by a float4 copy kernel on this part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--fractions", default="0.1,0.5")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--search-list", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_compact_probe.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mse
    from bench_ann import D, HARD_PARAMS, HardSet, recall_at
    n, nq, L, K, R, BATCH = a.rows, a.queries, a.search_list, 10, 64, 16384
    cfg = mse.IndexBuildConfig(r=R, l=192, maxc=750)
    hs = HardSet(n, **HARD_PARAMS)
    rows = hs.rows(n, 1)
    held = hs.rows(nq, 3)
    q16 = held.cpu().numpy().view(np.uint16)
    torch.cuda.synchronize()
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, D, keepalive=rows)
    s = mse.Searcher(vecs)
    t0 = time.perf_counter()
    g0 = mse.BuildGraph(n, R)
    g0.random_fill(1)
    g0.build(s, np.random.default_rng(1).permutation(n).astype(np.uint32), mse.medioid(vecs), cfg, BATCH)
    t_build = time.perf_counter() - t0
    h0 = g0.to_host()
    g0.close()
    out = {"set": "hard", "rows": n, "queries": nq, "search_list": L, "beamwidth": 4, "k": K, "copy_rate_bytes_per_s": COPY_RATE,
           "build": {"r": R, "l": 192, "maxc": 750, "passes": 1, "batch": BATCH, "seconds": t_build}, "fractions": []}

    def timed(run, count=nq):
        run()
        t = time.perf_counter()
        top = run()
        return top, count / (time.perf_counter() - t)

    def scan_ms(srch):
        srch.bruteforce_topk(q16[:128], K, mse.MODE_MFMA)
        t = time.perf_counter()
        srch.bruteforce_topk(q16[:128], K, mse.MODE_MFMA)
        return (time.perf_counter() - t) * 1e3

    for frac in [float(x) for x in a.fractions.split(",")]:
        rng = np.random.default_rng(int(frac * 1000) + 7)
        dead = rng.random(n) < frac
        live_ids = np.flatnonzero(~dead).astype(np.uint32)
        entries = np.sort(rng.choice(live_ids, max(4096, n // 1500), replace=False)).astype(np.uint32)
        _, truth = s.bruteforce_topk(q16, K, allow=mse.RowFilter(~dead))
        g = mse.BuildGraph(n, R, h0)
        mse.set_entries(g, vecs, entries)
        g.delete_rows(s, mse.RowFilter(dead), cfg)
        top, qps = timed(lambda: mse.disk_query_topk(s, None, None, g, q16, K, None, None, None, True, 4, L)[0])
        row = {"deleted_fraction": frac, "deleted_rows": int(dead.sum()), "before": {"recall_at_10": recall_at(top, truth), "queries_per_s": qps,
               "bruteforce_128_ms": scan_ms(s)}, "capacities": []}
        # the host round trip the call replaces
        t0 = time.perf_counter()
        h = g.to_host()
        host_rows = vecs.rows(0, n)
        o2n = np.full(n, 0xFFFFFFFF, np.uint32)
        o2n[live_ids] = np.arange(len(live_ids), dtype=np.uint32)
        new_deg = h.deg[live_ids]
        new_adj = np.where(np.arange(R)[None, :] < new_deg[:, None], o2n[np.minimum(h.adj[live_ids], n - 1)], 0).astype(np.uint32)
        up_v = mse.VectorList.from_f16s(host_rows[live_ids], D)
        up_g = mse.BuildGraph(len(live_ids), R, mse.IndexGraph(new_adj, new_deg))
        row["host_round_trip_seconds"] = time.perf_counter() - t0
        up_g.close()
        up_v.close()
        del host_rows, new_adj, h
        for cap in (len(live_ids), int(1.25 * n)):
            torch.cuda.synchronize()
            s.compact_timing(2)
            t0 = time.perf_counter()
            nv, _, ng, o2n_dev, _ = g.compact(s, capacity=cap)
            dt = time.perf_counter() - t0
            gather_ms = s.compact_timing(0)
            st = ng.compact_stats
            ns = mse.Searcher(nv)
            mse.set_entries(ng, nv, o2n_dev[entries])
            top, qps = timed(lambda: mse.disk_query_topk(ns, None, None, ng, q16, K, None, None, None, True, 4, L)[0])
            mapped = np.where(top == 0xFFFFFFFF, 0xFFFFFFFF, live_ids[np.minimum(top, len(live_ids) - 1)])
            gather_bytes = st["bytes_moved"] + cap * D * 2      # read: the live rows; written: every row of the new base, the zero tail included
            rate = gather_bytes / (gather_ms * 1e-3)
            row["capacities"].append(dict(st, seconds=dt, gather_ms=gather_ms, gather_bytes=gather_bytes, gather_bytes_per_s=rate,
                                          gather_fraction_of_copy_rate=rate / COPY_RATE,
                                          after={"recall_at_10": recall_at(mapped, truth), "queries_per_s": qps, "bruteforce_128_ms": scan_ms(ns)}))
            ng.close()
            ns.close()
            nv.close()
        g.close()
        out["fractions"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:          # after every fraction: a run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
