"""Grouped graph search: what the group step costs on the request path.

On bench_ann.py's hard set (1e7 rows by default), a Vamana graph as graph_index_bench builds it, exactly scored neighbours, entry by
4096+ sampled rows, L = 200, k = 10, beam 4.  For 1, 64 and 4096 queries per call the ungrouped call is timed against the grouped call
under three groupings -- every row NONE, runs of 8 rows, one group holding 90 % of the rows -- with the calls ALTERNATED inside one
loop and medians taken; the comparison is always the ungrouped call of the same round, never another grouped run.  Also recorded: how
many queries came back short (padding) under each grouping.  Nothing is asserted: the numbers go to profiles/grouped_graph_probe.json.

    python scripts/grouped_graph_probe.py [--rows 1e7] [--rounds 7] [--search-list 200] [--out FILE]
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


def probe(n, L, rounds, K=10, R=64, beam=4):
    import numpy as np
    import torch
    import mse
    import bench_ann as ba
    hs = ba.HardSet(n, **getattr(ba, "HARD_PARAMS", {}))
    rows, queries = hs.rows(n, 1), hs.rows(4096, 3)
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
    rng = np.random.default_rng(9)
    ninety = np.full(n, mse.GROUP_NONE, np.uint32)
    ninety[rng.random(n) < 0.9] = 0
    groupings = {"all_none": np.full(n, mse.GROUP_NONE, np.uint32), "runs_of_8": (np.arange(n, dtype=np.uint32) // 8) * 8,
                 "one_group_90pct": ninety}
    groupings = {name: mse.RowGroups(a) for name, a in groupings.items()}
    out = {"rows": n, "search_list": L, "k": K, "beamwidth": beam, "rounds": rounds, "build_seconds": build_s, "calls": []}
    for nq in (1, 64, 4096):
        q = q16[:nq]

        def run(groups):
            t0 = time.perf_counter()
            ids, _, _ = mse.disk_query_topk(s, None, None, g, q, K, None, None, None, True, beam, L, groups=groups)
            return (time.perf_counter() - t0) * 1e3, ids

        for groups in (None, *groupings.values()):                        # warm every form
            run(groups)
        ms = {name: [] for name in ("ungrouped", *groupings)}
        short = {}
        for _ in range(rounds):                                           # alternated: every round runs every form once
            ms["ungrouped"].append(run(None)[0])
            for name, groups in groupings.items():
                dt, ids = run(groups)
                ms[name].append(dt)
                short[name] = int((ids == mse.ID_NONE).any(axis=1).sum())
        row = {"queries_per_call": nq, "ungrouped_ms_median": statistics.median(ms["ungrouped"]), "ungrouped_ms": ms["ungrouped"], "grouped": {}}
        for name in groupings:
            row["grouped"][name] = {"ms_median": statistics.median(ms[name]), "ms": ms[name],
                                    "extra_ms_over_ungrouped": statistics.median(ms[name]) - row["ungrouped_ms_median"],
                                    "queries_short": short[name]}
        out["calls"].append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--search-list", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_graph_probe.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  -- before libmse_hip.so: the torch wheel bundles its own HIP runtime
    res = probe(int(a.rows), a.search_list, a.rounds)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
