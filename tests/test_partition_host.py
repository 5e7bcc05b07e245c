"""The shard partition (include/mse.h mse_partitioner), the part that needs no device: the refusals that happen before anything is
allocated, the prototypes against the header, and the restatement (tests/partition_ref.py) against its own definitions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import partition_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_SYMBOLS = ["mse_partition_set_sample_f16", "mse_partition_set_sample_base", "mse_partition_anneal", "mse_partition_state",
               "mse_partition_trace", "mse_partition_centroids", "mse_partition_set_centroids", "mse_partition_count", "mse_partition_scores",
               "mse_partition_assign_f16", "mse_partition_assign_base", "mse_partition_assign_reset", "mse_partition_assignment",
               "mse_partition_counts", "mse_partition_timing", "mse_medioid_ids", "mse_debug_partition_noise", "mse_debug_partition_normalise",
               "mse_debug_partition_chunk_rows"]


def declaration(text, name, ret=r"int"):
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_prototypes_match_the_header():
    from mse import ffi
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    sig = ffi.SIGNATURES
    for name in INT_SYMBOLS:
        assert sig[name][0] is C.c_int, name
        assert len(declaration(text, name)) == len(sig[name][1]), name
        assert getattr(ffi.lib(), name) is not None, name
    assert len(declaration(text, "mse_partition_new", r"mse_partitioner\*")) == len(sig["mse_partition_new"][1]) == 3
    assert len(declaration(text, "mse_partition_shard_filter", r"mse_filter\*")) == len(sig["mse_partition_shard_filter"][1]) == 2
    assert sig["mse_partition_new"][0] is C.c_void_p and sig["mse_partition_shard_filter"][0] is C.c_void_p
    assert len(declaration(text, "mse_partition_free", "void")) == 1 and len(declaration(text, "mse_partition_config_default", "void")) == 1
    # the structures, field for field
    for struct, cls in (("mse_partition_config", ffi.PartitionConfig), ("mse_partition_status", ffi.PartitionState)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], struct
    cfg = ffi.PartitionConfig()
    ffi.lib().mse_partition_config_default(C.byref(cfg))
    got = {k: getattr(cfg, k) for k, _ in ffi.PartitionConfig._fields_}
    assert got == {k: (float(np.float32(v)) if isinstance(v, float) and k != "stop_fraction" else v) for k, v in ref.DEFAULTS.items()}


def test_refusals_before_allocation(mse):
    from mse import ffi
    L = ffi.lib()
    for S, d, word in ((1, 1152, "shards"), (0, 1152, "shards"), (65, 1152, "shards"), (6, 1150, "multiple of 8"), (6, 0, "multiple of 8")):
        assert not L.mse_partition_new(S, d, None)
        assert word in ffi.last_error()
    bad = ffi.PartitionConfig()
    L.mse_partition_config_default(C.byref(bad))
    bad.stop_fraction = -1.0
    assert not L.mse_partition_new(6, 1152, C.byref(bad)) and "annealing" in ffi.last_error()
    with pytest.raises(mse.MseError):
        mse.ShardPartitioner(65)
    with pytest.raises(TypeError):
        mse.ShardPartitioner(6, heat=2.0)
    # a handle is made without a device; what can be refused from the arguments and the handle's state is refused first
    p = mse.ShardPartitioner(6, 1152, seed=1)
    rows = np.zeros((5, 1152), np.uint16)
    rp, out8, out64 = rows.ctypes.data_as(ffi.u16p), np.zeros(16, np.uint8), np.zeros(16, np.uint64)
    assert L.mse_partition_set_sample_f16(p._h, rp, 5) != 0 and "fewer rows than shards" in ffi.last_error()
    assert L.mse_partition_set_sample_f16(p._h, None, 100) != 0 and "null rows" in ffi.last_error()
    assert L.mse_partition_set_sample_base(p._h, None, None, 100) != 0 and "null base" in ffi.last_error()
    assert L.mse_partition_anneal(p._h, 1) != 0 and "no sample" in ffi.last_error()
    assert L.mse_partition_assign_f16(p._h, rp, 5, 0.2) != 0 and "no centroids" in ffi.last_error()
    assert L.mse_partition_assign_base(p._h, None, 0, 5, 0.2) != 0 and "null base" in ffi.last_error()
    assert L.mse_partition_set_centroids(p._h, None) != 0 and "null centroids" in ffi.last_error()
    assert L.mse_partition_count(p._h, None, None, None) != 0 and "null" in ffi.last_error()
    assert L.mse_partition_centroids(p._h, None, None, None) != 0 and "has not run" in ffi.last_error()
    assert not L.mse_partition_shard_filter(p._h, 6) and "not below 6" in ffi.last_error()
    assert not L.mse_partition_shard_filter(p._h, 0) and "no rows assigned" in ffi.last_error()
    assert L.mse_partition_assignment(p._h, 0, 1, out8.ctypes.data_as(ffi.u8p)) != 0 and "past the 0 rows" in ffi.last_error()
    n = C.c_uint64(7)
    assert L.mse_partition_counts(p._h, out64.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)) == 0 and n.value == 0 and not out64.any()
    with pytest.raises(mse.MseError):
        p.assign(rows)
    p.close()
    for rc in (L.mse_partition_set_sample_f16(None, rp, 5), L.mse_partition_set_sample_base(None, None, None, 0), L.mse_partition_anneal(None, 1),
               L.mse_partition_trace(None, 0, 0, None, None), L.mse_partition_centroids(None, None, None, None),
               L.mse_partition_set_centroids(None, None), L.mse_partition_count(None, None, None, None), L.mse_partition_scores(None, None, None),
               L.mse_partition_assign_f16(None, rp, 5, 0.2), L.mse_partition_assign_base(None, None, 0, 0, 0.2), L.mse_partition_assign_reset(None),
               L.mse_partition_assignment(None, 0, 0, None), L.mse_partition_counts(None, None, None), L.mse_debug_partition_chunk_rows(None, 1)):
        assert rc != 0 and "null partitioner" in ffi.last_error()
    assert L.mse_partition_state(None, None) != 0 and L.mse_partition_timing(None, None) != 0
    assert not L.mse_partition_shard_filter(None, 0) and "null partitioner" in ffi.last_error()
    L.mse_partition_free(None)
    u32 = np.zeros(1, np.uint32)
    assert L.mse_medioid_ids(None, u32.ctypes.data_as(ffi.u32p), 1, u32.ctypes.data_as(ffi.u32p)) != 0 and "null" in ffi.last_error()
    f = np.zeros(8, np.float32)
    assert L.mse_debug_partition_noise(1, 0, 12, f.ctypes.data_as(ffi.f32p)) != 0 and "multiple of 8" in ffi.last_error()
    assert L.mse_debug_partition_normalise(f.ctypes.data_as(ffi.f32p), 0, 8, f.ctypes.data_as(ffi.f32p), None) != 0


def test_restatement_against_its_definitions(orc):
    """The noise has unit variance and the stated bound; the Newton square root agrees with sqrt to an ulp over the range a centroid's
    sum of squares can take; the walk with no fudge picks the two largest scaled scores; the stop test is the integer one."""
    z = np.concatenate([ref.noise(orc, 3, k, 1152) for k in range(64)]).astype(np.float64)
    assert abs(z.var() - 1.0) < 0.02 and abs(z.mean()) < 0.02 and np.abs(z).max() <= 131070 * float(ref.K) < 3.47
    for ss in (1e-24, 3.7e-5, 1.0, 1152.0, 2.5e6, 1e20):
        c = np.zeros((1, 8), np.float32)
        c[0, 0] = np.float32(np.sqrt(ss))
        got = ref.normalise(c)[0, 0]
        assert got == np.float32(1.0), ss
    rng = np.random.default_rng(1)
    sc = rng.standard_normal((50, 5)) * 0.1
    a, counts, bal = ref.walk(sc, 0.0)
    order = np.argsort(-sc, axis=1, kind="stable")[:, :2]
    assert np.array_equal(a, order) and counts.sum() == 100 and bal == 51
    a2, c2, b2 = ref.walk(sc[:20], 0.3)
    a3, c3, b3 = ref.walk(sc[20:], 0.3, c2, b2)
    full = ref.walk(sc, 0.3)
    assert np.array_equal(np.concatenate([a2, a3]), full[0]) and np.array_equal(c3, full[1]) and b3 == full[2]
    assert ref.fitness(np.array([[3, 1, 2], [2, 2, 2]], np.uint64), 6) == (3, [0, 0])
    assert ref.fitness(np.array([[2, 2, 2], [0, 3, 3]], np.uint64), 6) == (6, [0, 0])
    assert list(ref.scale_dot_result_f64(np.array([0.5, -0.5, 1e30, -1e30, np.nan]))) == [1 << 31, -(1 << 31), 2 ** 63 - 1, -2 ** 63, 0]
