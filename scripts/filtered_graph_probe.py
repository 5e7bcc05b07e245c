"""Filtered graph search: queries/s and recall@10 of the three regimes per allowed fraction.

On bench_ann.py's hard and easy sets (1e7 rows by default), a Vamana graph as graph_index_bench builds it, exactly scored neighbours,
entry by 4096+ sampled rows.  Filters: uniformly random rows at fractions 0.5 .. 1e-4, and one clustered filter per set (every row
within a dot-product radius of a few sampled rows, sized to ~2 % of the rows: the adversarial case for a traversal).  For each:
GRAPH at L' = ceil(L n / c) (skipped past 1024), LIST, and AUTO, against mse_bruteforce_topk_filtered_f16's answer.  Nothing is
asserted: the numbers go to profiles/filtered_graph_probe.json (and DESIGN 3.9).

    python scripts/filtered_graph_probe.py [--rows 1e7] [--kinds hard,easy] [--queries 1024] [--search-list 64] [--out FILE]
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

FRACTIONS = (0.5, 0.2, 0.1, 0.05, 0.02, 0.01, 1e-3, 1e-4)


def timed(fn, repeat=2):
    fn()                                                                  # warm
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return out, best


def probe_set(kind, n, nq, L, K=10, R=64, beam=4):
    import numpy as np
    import torch
    import mse
    import bench_ann as ba
    if kind == "easy":
        gen = ba.easy_generator(n)
        rows, queries = gen(n, 1), gen(nq, 3)
    else:
        hs = ba.HardSet(n, **getattr(ba, "HARD_PARAMS", {}))
        rows, queries = hs.rows(n, 1), hs.rows(nq, 3)
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
    q16 = queries.cpu().numpy().view(np.uint16)
    rng = np.random.default_rng(8)
    masks = [("uniform", f, rng.random(n) < f) for f in FRACTIONS]
    # clustered: the rows closest to a few sampled rows, ~2 % of the base
    seeds = rows[torch.from_numpy(rng.choice(n, 8, replace=False)).cuda()].float()
    best = torch.empty(n, device="cuda")
    for i in range(0, n, 1 << 20):
        best[i:i + (1 << 20)] = (rows[i:i + (1 << 20)].float() @ seeds.T).max(dim=1).values
    cut = torch.quantile(best[torch.randint(0, n, (1 << 20,), device="cuda")], 0.98)
    masks.append(("clustered", 0.02, (best >= cut).cpu().numpy()))
    out = {"kind": kind, "rows": n, "queries": nq, "search_list": L, "beamwidth": beam, "build_seconds": build_s, "filters": []}
    for shape, frac, mask in masks:
        flt = mse.RowFilter(mask)
        c = flt.count
        _, truth = s.bruteforce_topk(q16, K, allow=flt)                  # mse_bruteforce_topk_filtered_f16
        plan = mse.filtered_plan(n, c, L)
        widened = -(-L * n // c) if c else None
        row = {"shape": shape, "fraction": frac, "allowed": c, "widened_search_list": widened, "plan": list(plan)}

        def run(regime, sl):
            return mse.disk_query_topk(s, None, None, g, q16, K, None, None, None, True, beam, sl, filter=flt, regime=regime)

        legs = [("list", "list", L), ("auto", "auto", L)]
        if widened is not None and widened <= 1024:
            legs.insert(0, ("graph_at_widened", "graph", max(L, widened)))
        for name, regime, sl in legs:
            try:
                (top, _, st), dt = timed(lambda: run(regime, sl))
                row[name] = {"search_list": sl, "queries_per_s": nq / dt, "recall_at_10": ba.recall_at(top, truth),
                             "node_fetches_per_query": float(st["cmps"].mean())}
            except mse.MseError as e:
                row[name] = {"error": str(e)}
        if "graph_at_widened" in row and "queries_per_s" in row["graph_at_widened"] and "queries_per_s" in row["list"]:
            faster = "graph" if row["graph_at_widened"]["queries_per_s"] >= row["list"]["queries_per_s"] else "list"
            row["faster_regime"], row["auto_picked_the_slower"] = faster, plan[0] != faster
        out["filters"].append(row)
        print(json.dumps(row), flush=True)
        flt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--kinds", default="hard,easy")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--search-list", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_graph_probe.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before libmse_hip.so: the torch wheel bundles its own HIP runtime
    res = {"sets": [probe_set(kind, int(a.rows), a.queries, a.search_list) for kind in a.kinds.split(",")]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
