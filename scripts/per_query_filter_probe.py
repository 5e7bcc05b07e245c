"""A filter per query within one launch: what a batch of requests with their own filters costs.

On bench_ann.py's hard set (1e7 rows by default), a Vamana graph as graph_index_bench builds it, exactly scored neighbours, entry by
4096+ sampled rows, L = 200, k = 10, beam 4, explicit GRAPH regime.  Every query has a filter object of its own that allows about half
of the rows (XORs of pairs of independent half masks, made on the device).  For 64 and 4096 queries, ALTERNATED inside one loop, medians
of `rounds`:

  each         the queries in ONE mse_disk_query_topk_filtered_each call: one launch, the kernel reads a filter per query
  one_filter   the same queries in one single-filter call (every query under the first filter): the ceiling
  lone_calls   one single-filter one-query call per query, one after the other from this thread: all that was possible before
  tickets_each / tickets_one_filter   the same through QueryTickets from one thread: a filter per request against one shared filter
                (before, tickets with distinct filter objects never shared a submission)

Nothing is asserted: the numbers go to profiles/per_query_filter_probe.json.

    python scripts/per_query_filter_probe.py [--rows 1e7] [--rounds 7] [--search-list 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "meme-search-engine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def probe(n, L, rounds, sizes=(64, 4096), K=10, R=64, beam=4):
    import numpy as np
    import torch
    import mse
    import bench_ann as ba
    hs = ba.HardSet(n, **getattr(ba, "HARD_PARAMS", {}))
    rows, queries = hs.rows(n, 1), hs.rows(max(sizes), 3)
    torch.cuda.synchronize()
    vecs = mse.VectorList.wrap_device(rows.data_ptr(), n, ba.D, keepalive=rows)
    s = mse.Searcher(vecs)
    t0 = time.perf_counter()
    g = mse.BuildGraph(n, R)
    g.random_fill(1)
    order = np.random.default_rng(3).permutation(n).astype(np.uint32)
    g.build(s, order, mse.medioid(vecs), mse.IndexBuildConfig(r=R, l=192, maxc=750), 16384)
    build_s = time.perf_counter() - t0
    mse.set_entries(g, vecs, np.sort(np.random.default_rng(5).choice(n, max(4096, n // 1500), replace=False)).astype(np.uint32))
    q32 = queries.float().cpu().numpy()
    # one filter object per query: m independent half masks from the host, their pairwise XORs (half masks again) on the device
    rng = np.random.default_rng(9)
    m = 2
    while m * (m - 1) // 2 < max(sizes):
        m += 1
    t0 = time.perf_counter()
    halves = [mse.RowFilter(rng.random(n) < 0.5) for _ in range(m)]
    filters = []
    for a in range(m):
        for b in range(a + 1, m):
            if len(filters) < max(sizes):
                filters.append(halves[a] ^ halves[b])
    filters_s = time.perf_counter() - t0
    out = {"rows": n, "search_list": L, "k": K, "beamwidth": beam, "rounds": rounds, "build_seconds": build_s, "filters": len(filters),
           "filters_seconds": filters_s, "allowed_fraction_first": filters[0].count / n, "calls": []}

    def topk(q, **kw):
        return mse.disk_query_topk(s, None, None, g, q, K, None, None, None, True, beam, L, regime="graph", **kw)

    def tickets(tk, q, flts):
        for i in range(len(q)):
            tk.submit(q[i], key=i, **({"filter": flts[i]} if flts is not None else {}))
        left = len(q)
        while left:
            left -= len(tk.collect(max_tickets=256, timeout_us=10_000_000))

    for nq in sizes:
        q, flts = q32[:nq], filters[:nq]
        tk_own = mse.QueryTickets(s, None, None, g, K, True, beam, L, regime="graph")
        tk_one = mse.QueryTickets(s, None, None, g, K, True, beam, L, filter=flts[0], regime="graph")
        forms = {"each": lambda: topk(q, filter=flts),
                 "one_filter": lambda: topk(q, filter=flts[0]),
                 "lone_calls": lambda: [topk(q[i:i + 1], filter=flts[i]) for i in range(nq)],
                 "tickets_each": lambda: tickets(tk_own, q, flts),
                 "tickets_one_filter": lambda: tickets(tk_one, q, None)}
        for run in forms.values():                                        # warm every form
            run()
        ms = {name: [] for name in forms}
        before = mse.coalescer_stats(g)
        for _ in range(rounds):                                           # alternated: every round runs every form once
            for name, run in forms.items():
                t0 = time.perf_counter()
                run()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        after = mse.coalescer_stats(g)
        row = {"queries": nq, "coalescer_requests": after["requests"] - before["requests"], "coalescer_passes": after["passes"] - before["passes"]}
        for name in forms:
            row[name] = {"ms_median": statistics.median(ms[name]), "ms": ms[name]}
        row["each_over_one_filter"] = row["each"]["ms_median"] / row["one_filter"]["ms_median"]
        row["lone_calls_over_each"] = row["lone_calls"]["ms_median"] / row["each"]["ms_median"]
        row["tickets_each_over_tickets_one_filter"] = row["tickets_each"]["ms_median"] / row["tickets_one_filter"]["ms_median"]
        out["calls"].append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--search-list", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_query_filter_probe.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before libmse_hip.so: the torch wheel bundles its own HIP runtime
    res = probe(int(a.rows), a.search_list, a.rounds)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
