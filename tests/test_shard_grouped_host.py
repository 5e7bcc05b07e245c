"""Grouped search across the shards (include/mse.h), the part that needs no device: the new entry points declared, exported and bound
with the argument order of the calls they extend, the canonical relabelling rule of mse_groups_slice and the identity the grouped merge
rests on -- collapse(merge of the per-shard grouped top-k) = collapse(merge of everything the shards ranked), cut to k -- restated in
numpy, and the benchmark's dry run untouched."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, LOWEST = 0xFFFFFFFF, np.iinfo(np.int64).min

NEW_SYMBOLS = ["mse_groups_slice", "mse_groups_read", "mse_shard_group_groups", "mse_shard_groups_part", "mse_shard_groups_n_shards",
               "mse_shard_groups_free", "mse_merge_topk_packed_grouped_dev", "mse_shard_group_search_grouped", "mse_shard_group_search_grouped_dev",
               "mse_shard_group_pq_scan_topk_grouped", "mse_shard_group_query_topk_grouped", "mse_disk_query_topk_block_grouped"]


def test_new_entry_points_are_declared_exported_and_bound():
    import mse
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in ffi.SIGNATURES, name
        assert getattr(ffi.lib(), name) is not None, name
    sig = ffi.SIGNATURES
    # every grouped call takes the arguments of its filtered sibling plus the shard groups, in front of the (now optional) shard filter
    for grouped, filtered in (("mse_shard_group_search_grouped", "mse_shard_group_search_filtered"),
                              ("mse_shard_group_search_grouped_dev", "mse_shard_group_search_filtered_dev"),
                              ("mse_shard_group_pq_scan_topk_grouped", "mse_shard_group_pq_scan_topk_filtered"),
                              ("mse_shard_group_query_topk_grouped", "mse_shard_group_query_topk_filtered")):
        g, f = sig[grouped], sig[filtered]
        assert g[0] == f[0] and g[1][0] == f[1][0] and g[1][1] == ffi.vp and g[1][2:] == f[1][1:], grouped
    # the block form: the filtered block form with the grouping in front of the filter
    g, f = sig["mse_disk_query_topk_block_grouped"], sig["mse_disk_query_topk_block_filtered"]
    assert g[1][:4] == f[1][:4] and g[1][4] == ffi.vp and g[1][5:] == f[1][4:]
    # the merge hook: the packed merge with the grouping after the searcher and k_in in front of k
    g, f = sig["mse_merge_topk_packed_grouped_dev"], sig["mse_merge_topk_packed_dev"]
    assert g[1] == [f[1][0], ffi.vp] + f[1][1:4] + [ffi.sz] + f[1][4:]
    assert sig["mse_groups_slice"] == sig["mse_filter_slice"]
    # the header declares the same argument order by name
    for name, order in (("mse_shard_group_search_grouped", ["g", "sg", "sf", "queries", "nq", "k", "mode", "scores", "ids"]),
                        ("mse_shard_group_pq_scan_topk_grouped", ["g", "sg", "sf", "queries_f32", "scales", "nq", "r", "k", "mode", "scores", "ids"]),
                        ("mse_shard_group_query_topk_grouped", ["g", "sg", "sf", "queries", "luts", "scales", "nq", "disable_pq", "beamwidth",
                                                                "search_list", "k", "regime", "scores", "ids"]),
                        ("mse_merge_topk_packed_grouped_dev", ["s", "groups_global", "gathered_blocks_dev", "n_shards", "nq", "k_in", "k",
                                                               "out_scores_dev", "out_ids_dev"])):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
        assert [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in decl.split(",")] == order, name
        assert len(order) == len(sig[name][1]), name
    for cls, names in ((mse.RowGroups, ("slice", "to_host")), (mse.ShardGroups, ("shard", "n_shards", "close")),
                       (mse.ShardGroup, ("groups", "bruteforce_topk_grouped", "bruteforce_topk_grouped_dev", "query_topk_grouped",
                                         "pq_scan_topk_grouped"))):
        for n in names:
            assert hasattr(cls, n), (cls.__name__, n)
    assert "has no grouped twin." not in text and "mse_disk_query_topk_block_grouped" in text


def canonical_slice(labels, first, n_rows):
    part = labels[first:first + n_rows]
    out = np.full(len(part), NONE, np.uint32)
    first_of = {}
    for i, g in enumerate(part.tolist()):
        if g != NONE:
            out[i] = first_of.setdefault(g, i)
    return out


def same_partition(a, b):
    """two label arrays induce the same partition (NONE rows are singletons in both)"""
    if len(a) != len(b) or not np.array_equal(a == NONE, b == NONE):
        return False
    pairs = {(int(x), int(y)) for x, y in zip(a, b) if x != NONE}
    return len({x for x, _ in pairs}) == len(pairs) == len({y for _, y in pairs})


def test_canonical_slice_rule_keeps_the_partition_and_is_a_fixed_point():
    rng = np.random.default_rng(7)
    n = 2999
    labels = rng.integers(0, 300, n).astype(np.uint32)
    labels[rng.random(n) < 0.1] = NONE
    for first, m in ((0, 750), (750, 750), (2250, 749), (1, 65), (2990, 64), (3000, 10)):
        out = canonical_slice(labels, first, m)
        assert len(out) == max(0, min(m, n - first))
        assert same_partition(out, labels[first:first + m])
        grouped = out != NONE
        assert (out[grouped] <= np.flatnonzero(grouped)).all() and (out[out[grouped]] == out[grouped]).all()     # a label is its group's first row
        assert np.array_equal(canonical_slice(out, 0, len(out)), out)


def collapse(scores, ids, labels, k):
    live = ids != NONE
    s, i = scores[live], ids[live].astype(np.int64)
    order = np.lexsort((i, ~s))
    s, i = s[order], i[order]
    lab = np.full(len(i), NONE, np.int64)
    inside = i < len(labels)
    lab[inside] = labels[i[inside]]
    _, firsts = np.unique(np.where(lab == NONE, (1 << 32) + i, lab), return_index=True)
    keep = np.sort(firsts)[:k]
    out_s, out_i = np.full(k, LOWEST, np.int64), np.full(k, NONE, np.uint32)
    out_s[:len(keep)], out_i[:len(keep)] = s[keep], i[keep]
    return out_s, out_i


@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("k", [1, 10, 200])
def test_k_records_per_shard_are_enough(G, k):
    """per shard: the grouped top-k under the shard's canonical slice of the grouping; merged and collapsed by the global grouping they
    give the collapse of all rows -- with scores full of ties, groups on every shard, one giant group, and a grouping shorter than the rows"""
    rng = np.random.default_rng(100 * G + k)
    n = 2999
    base, rem = divmod(n, G)
    bounds = [(g * base + min(g, rem), g * base + min(g, rem) + base + (1 if g < rem else 0)) for g in range(G)]
    scattered = rng.integers(0, 300, n).astype(np.uint32)
    giant = np.full(n, NONE, np.uint32)
    giant[rng.choice(n, n * 9 // 10, replace=False)] = 5
    for labels in (scattered, giant, scattered[:1600], np.full(n, NONE, np.uint32)):
        scores = rng.integers(-5, 5, n).astype(np.int64)
        ids = np.arange(n, dtype=np.uint32)
        want = collapse(scores, ids, labels, k)
        parts_s, parts_i = [], []
        for lo, hi in bounds:
            local = canonical_slice(labels, lo, hi - lo)
            s, i = collapse(scores[lo:hi], np.arange(hi - lo, dtype=np.uint32), local, k)
            parts_s.append(s)
            parts_i.append(np.where(i == NONE, i, i + np.uint32(lo)))
        got = collapse(np.concatenate(parts_s), np.concatenate(parts_i), labels, k)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_bench_dry_run_is_unaffected():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", "--gpus", "8"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 8 and line["value"] is None and "dry-run" in line["data"]
    assert line["config"]["parallelism"] == "row-shard x8" and "grouped" not in json.dumps(line)
