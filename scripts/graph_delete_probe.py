"""Delete-and-repair against a rebuild, on the hard synthetic set of bench_ann.py (not bench.py; nothing imports this).

For each deleted fraction: the time of DeviceGraph/BuildGraph.delete_rows against a one-pass rebuild over the live rows, and held-out
recall@10 / queries per second at search list 200 for three ways of living with the deletes:
  lazy      the untouched graph searched with an allowed-row filter (dead nodes are walked through and dropped from the answer)
  repaired  the graph after delete_rows
  rebuilt   a new graph over the live rows only (ids mapped back)
Writes profiles/graph_delete_probe.json.  Needs one MI355X.

    python scripts/graph_delete_probe.py [--rows 10000000] [--fractions 0.01,0.1,0.5]
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
    ap.add_argument("--fractions", default="0.01,0.1,0.5")
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--search-list", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_delete_probe.json"))
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

    def build(vl, srch, m, seed):
        t0 = time.perf_counter()
        g = mse.BuildGraph(m, R)
        g.random_fill(seed)
        g.build(srch, np.random.default_rng(seed).permutation(m).astype(np.uint32), mse.medioid(vl), cfg, BATCH)
        return g, time.perf_counter() - t0

    g0, t_build = build(vecs, s, n, 1)
    h0 = g0.to_host()
    g0.close()
    out = {"set": "hard", "rows": n, "queries": nq, "search_list": L, "beamwidth": 4, "k": K, "build": {"r": R, "l": 192, "maxc": 750, "passes": 1,
           "batch": BATCH, "seconds": t_build}, "fractions": []}

    def timed(run):
        run()
        t0 = time.perf_counter()
        top = run()
        return top, nq / (time.perf_counter() - t0)

    for frac in [float(x) for x in a.fractions.split(",")]:
        rng = np.random.default_rng(int(frac * 1000) + 7)
        dead = rng.random(n) < frac
        live_ids = np.flatnonzero(~dead).astype(np.uint32)
        entries = np.sort(rng.choice(live_ids, max(4096, n // 1500), replace=False)).astype(np.uint32)
        live_filter = mse.RowFilter(~dead)
        _, truth = s.bruteforce_topk(q16, K, allow=live_filter)
        row = {"deleted_fraction": frac, "deleted_rows": int(dead.sum())}
        # lazy: the untouched graph behind the allowed-row filter
        g = mse.BuildGraph(n, R, h0)
        mse.set_entries(g, vecs, entries)
        top, qps = timed(lambda: mse.disk_query_topk(s, None, None, g, q16, K, None, None, None, True, 4, L, filter=live_filter, regime="graph")[0])
        row["lazy_by_filter"] = {"recall_at_10": recall_at(top, truth), "queries_per_s": qps}
        # repaired
        dead_filter = mse.RowFilter(dead)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = g.delete_rows(s, dead_filter, cfg)
        row["delete_rows"] = dict(st, seconds=time.perf_counter() - t0)
        top, qps = timed(lambda: mse.disk_query_topk(s, None, None, g, q16, K, None, None, None, True, 4, L)[0])
        row["repaired"] = {"recall_at_10": recall_at(top, truth), "queries_per_s": qps}
        g.close()
        # rebuilt over the live rows
        live_rows = rows[torch.from_numpy(live_ids.astype(np.int64)).cuda()].contiguous()
        lv = mse.VectorList.wrap_device(live_rows.data_ptr(), len(live_ids), D, keepalive=live_rows)
        ls = mse.Searcher(lv)
        g2, t_re = build(lv, ls, len(live_ids), 2)
        row["rebuild_seconds"] = t_re
        pos = np.searchsorted(live_ids, entries).astype(np.uint32)
        mse.set_entries(g2, lv, pos)
        top, qps = timed(lambda: mse.disk_query_topk(ls, None, None, g2, q16, K, None, None, None, True, 4, L)[0])
        mapped = np.where(top == 0xFFFFFFFF, 0xFFFFFFFF, live_ids[np.minimum(top, len(live_ids) - 1)])
        row["rebuilt"] = {"recall_at_10": recall_at(mapped, truth), "queries_per_s": qps}
        row["repair_over_rebuild_time"] = row["delete_rows"]["seconds"] / t_re
        g2.close()
        del live_rows, lv, ls
        out["fractions"].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:          # after every fraction: a run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
