"""The selection every search ends in -- descend() (api.hip) over reduce_max / reduce_max_gq / select_kernel (topk.hip) -- on keys no
search produces, through mse_debug_select_topk, and the two public merges on arbitrary gathered records.

Whole searches only ever hand the tournament 32.32 fixed-point dot products of near-unit vectors: a band narrower than 2^33 that agrees
on its top three bytes and almost never ties.  Here the keys are chosen for the kernel's data-dependent paths instead: no agreed digit,
keys straddling the sign bit, tie runs longer than the 4096-entry LDS list across many 256-entry groups, keys that differ in their
lowest byte only, saturated values, +-0 / +-inf / denormals, k at 2047 and 2048, k > n, and n on both sides of every level boundary
(16384 | 16385: one level | two; 4,194,304 | 4,194,305: two | three).

Reference: plain numpy, below.  Order is (key descending, id ascending); for floats that is IEEE total order (-0.0 below +0.0).
NaN keys are out of scope: the kernel orders their bit patterns, which no caller relies on.

mse_debug_select_topk also returns what descend() leaves in last_kth, the floor of the PQ scan's next select.  The contract pinned here
is the one that floor needs: last_kth <= the k-th best key (so at least k entries reach it), 0 when fewer than k entries exist.  It is
NOT always the k-th key itself: the radix search stops as soon as a bucket is taken whole and leaves the lower digits zero."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest

from conftest import SEED_BASE

KIND_I64, KIND_F32, KIND_U32 = 0, 1, 3               # KeyKind (csrc/kernels.h)
DT = {KIND_I64: np.int64, KIND_F32: np.float32, KIND_U32: np.uint32}
BITS = {KIND_I64: np.uint64, KIND_F32: np.uint32, KIND_U32: np.uint32}
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
FLT_MAX = np.finfo(np.float32).max
PAD_KEY = {KIND_I64: I64_MIN, KIND_F32: -np.inf, KIND_U32: 0}
WINNING_PAD = {KIND_I64: I64_MAX, KIND_F32: np.inf, KIND_U32: 0xFFFFFFFF}   # what a padding column holds: it would win if read
ID_NONE = 0xFFFFFFFF
KMAX = 2048                                          # TOPK_KMAX
TWO_LEVELS, THREE_LEVELS = 16385, 4_194_305          # DENSE_MAX + 1, DENSE_MAX * 256 + 1


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def sortable(keys, kind):
    """Order-preserving unsigned image of the keys (u64 for i64 keys, u32 otherwise)."""
    keys = np.ascontiguousarray(keys, DT[kind])
    if kind == KIND_I64:
        return keys.view(np.uint64) ^ np.uint64(1 << 63)
    if kind == KIND_F32:
        b = keys.view(np.uint32)
        return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return keys


def reference_order(keys_row, kind, k):
    """ids of the k best entries of one query: key descending, id ascending"""
    return np.argsort(~sortable(keys_row, kind), kind="stable")[:k]


def kth_domain(key_u, kind):
    """a sortable key as descend() reports it: u64, 32-bit keys in the top half"""
    return key_u.astype(np.uint64) << np.uint64(0 if kind == KIND_I64 else 32)


def merge_reference(scores, ids, k):
    """[nq][m] gathered records -> [nq][k] by (score descending, id ascending); records with id ID_NONE are absent"""
    nq = scores.shape[0]
    out_s = np.full((nq, k), I64_MIN, np.int64)
    out_i = np.full((nq, k), ID_NONE, np.uint32)
    for q in range(nq):
        valid = np.flatnonzero(ids[q] != ID_NONE)
        by_id = valid[np.argsort(ids[q][valid], kind="stable")]
        best = by_id[reference_order(scores[q][by_id], KIND_I64, k)]
        out_s[q, :best.size] = scores[q][best]
        out_i[q, :best.size] = ids[q][best]
    return out_s, out_i


# ---- key families (each: rng, kind, nq, n, k -> keys [nq][n]) -------------------------------------------------------------------------

def plant(keys, vals):
    """vals at known, evenly spread ids (the same in every query)"""
    n = keys.shape[1]
    for j, v in enumerate(vals):
        keys[:, (n * (2 * j + 1)) // (2 * len(vals))] = v
    return keys


def fam_full(rng, kind, nq, n, k):
    """full range: no digit agreed, top byte differs, the extremes planted (twice: they tie)"""
    if kind == KIND_I64:
        return plant(rng.integers(I64_MIN, I64_MAX, size=(nq, n), dtype=np.int64, endpoint=True), [I64_MIN, I64_MAX, 0, -1, I64_MAX, I64_MIN])
    if kind == KIND_U32:
        return plant(rng.integers(0, 2 ** 32, size=(nq, n), dtype=np.uint32), [0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 0])
    bits = rng.integers(0, 2 ** 32, size=(nq, n), dtype=np.uint32)
    bits[(bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)] &= np.uint32(0xFF000000)   # no NaN, no inf: those exponents become the largest finite one
    return bits.view(np.float32)


def fam_bands(rng, kind, nq, n, k):
    """width 2^20 above a large positive value and above a large negative one (every score digit but the low three agreed, and not
    zero), and a band straddling 0 (-1 and 0 differ in every byte of the sortable key: nothing agreed)"""
    centres = [0x4123456789000000, -0x4123456789000000, -2 ** 19]
    keys = rng.integers(0, 2 ** 20, size=(nq, n), dtype=np.int64)
    for q in range(nq):
        keys[q] += centres[q % 3]
    return keys


def fam_equal(rng, kind, nq, n, k):
    consts = {KIND_I64: [777, I64_MIN, I64_MAX, 0, -1], KIND_U32: [777, 0, 0xFFFFFFFF, 0x80000000], KIND_F32: [1.5, -0.0, 0.0, -np.inf]}[kind]
    keys = np.empty((nq, n), DT[kind])
    for q in range(nq):
        keys[q] = consts[q % len(consts)]
    return keys


def fam_two_values(rng, kind, nq, n, k):
    """k // 2 entries of the higher value, the lower one everywhere else: the k-th entry lies inside a tie run of n - k // 2"""
    pairs = [(-5, 3 << 40), (I64_MIN, I64_MIN + 1), (-1, 0)]
    keys = np.empty((nq, n), np.int64)
    for q in range(nq):
        lo, hi = pairs[q % 3]
        keys[q] = lo
        keys[q, rng.choice(n, k // 2, replace=False)] = hi
    return keys


def fam_low_byte(rng, kind, nq, n, k):
    bases = {KIND_I64: [0x1234567890ABCD00, -0x1234567890ABCD00, 0, -256], KIND_U32: [0xABCDEF00, 0, 0x7FFFFF00, 0xFFFFFF00]}[kind]
    keys = rng.integers(0, 256, size=(nq, n)).astype(DT[kind])
    for q in range(nq):
        keys[q] |= DT[kind](bases[q % len(bases)])
    return keys


def fam_ascending(rng, kind, nq, n, k):
    """distinct keys around 0, best entries last (in the short last group when n is no multiple of 256)"""
    return np.stack([(np.arange(n, dtype=np.int64) - n // 2) * (q + 1) + q for q in range(nq)])


def fam_descending(rng, kind, nq, n, k):
    return np.ascontiguousarray(fam_ascending(rng, kind, nq, n, k)[:, ::-1])


def fam_one_group(rng, kind, nq, n, k):
    """the k best all inside one 256-group"""
    assert k <= 256 <= n
    keys = rng.integers(-2 ** 40, 2 ** 40, size=(nq, n), dtype=np.int64)
    for q in range(nq):
        g = (n // 256 // 2 + q) % (n // 256)
        keys[q, g * 256 + rng.choice(256, k, replace=False)] = 2 ** 50 + rng.integers(0, 2 ** 30, k)
    return keys


def fam_one_per_group(rng, kind, nq, n, k):
    """exactly one of the k best in each of k groups"""
    assert k <= n // 256
    keys = rng.integers(0, 2 ** 30, size=(nq, n), dtype=np.int64)
    for q in range(nq):
        groups = rng.choice(n // 256, k, replace=False)
        keys[q, groups * 256 + rng.integers(0, 256, k)] = 2 ** 40 + rng.integers(0, 2 ** 20, k)
    return keys


def fam_shared_group_max(rng, kind, nq, n, k):
    """every full group holds the value V once (more than k groups share the k-th group maximum); k // 2 of them a larger value too"""
    g_full = n // 256
    assert g_full > k
    keys = rng.integers(-2 ** 30, 0, size=(nq, n), dtype=np.int64)
    for q in range(nq):
        keys[q, np.arange(g_full) * 256 + rng.integers(0, 128, g_full)] = 1000
        keys[q, rng.choice(g_full, k // 2, replace=False) * 256 + 128 + rng.integers(0, 128, k // 2)] = 2 ** 33 + rng.integers(0, 2 ** 20, k // 2)
    return keys


def fam_f32_special(rng, kind, nq, n, k):
    """+-0.0, +-inf, denormals, +-FLT_MAX among normal values; every third query only +-0.0, every third only denormals"""
    keys = (rng.standard_normal((nq, n)) * 8).astype(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, -FLT_MAX, FLT_MAX, np.finfo(np.float32).tiny], np.float32)
    for q in range(nq):
        if q % 3 == 1:
            keys[q] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
        elif q % 3 == 2:
            keys[q] = (rng.integers(1, 0x800000, n, dtype=np.uint32) | (rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31))).view(np.float32)
        for v in specials:
            keys[q, rng.integers(0, n, n // 64 + 1)] = v
    return keys


def fam_f32_copies(rng, kind, nq, n, k):
    """k // 2 larger values, then 5000 copies of one value around the k-th place, the rest below"""
    assert n >= k // 2 + 5000
    keys = (np.float32(0.499) - rng.random((nq, n)).astype(np.float32)).astype(np.float32)
    for q in range(nq):
        p = rng.permutation(n)
        keys[q, p[:k // 2]] = np.float32(0.501) + rng.random(k // 2).astype(np.float32)
        keys[q, p[k // 2:k // 2 + 5000]] = np.float32(0.5)
    return keys


def fam_floor_overflow(rng, kind, nq, n, k):
    """two adjacent values, half and half, in every group, and a third in each of the last k // 2 groups: fewer than k group maxima
    exceed the middle value, so it is the floor handed down -- and about 128 x k children reach it, far more than the 4096 the
    LDS list holds.  The k best are spread over all k parents."""
    g_full = n // 256
    assert g_full > k >= 64
    level = (rng.random((nq, n)) < 0.5).astype(np.int64)
    for q in range(nq):
        level[q, (g_full - 1 - np.arange(k // 2)) * 256 + rng.integers(0, 256, k // 2)] = 2
    if kind == KIND_F32:
        return (np.float32(1.0) + level.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    return level - 2 ** 45


CASES = [
    # one level (n <= 16384): one dense select
    ("full", KIND_I64, fam_full, 1, 3, (1, 2, 2048)),
    ("full", KIND_I64, fam_full, 255, 9, (1, 255, 256, 2048)),
    ("full", KIND_I64, fam_full, 256, 3, (2, 255, 256, 257)),
    ("full", KIND_I64, fam_full, 257, 9, (1, 256, 257, 2047)),
    ("full", KIND_I64, fam_full, 16384, 3, (1, 2, 255, 2047, 2048)),
    ("full", KIND_U32, fam_full, 257, 3, (2, 257, 2048)),
    ("full", KIND_U32, fam_full, 16384, 9, (256, 2048)),
    ("full", KIND_F32, fam_full, 16384, 3, (1, 2047)),
    ("bands", KIND_I64, fam_bands, 16384, 3, (1, 257, 2048)),
    ("equal", KIND_I64, fam_equal, 257, 9, (2, 256, 2048)),
    ("equal", KIND_I64, fam_equal, 16384, 3, (1, 256, 2048)),
    ("equal", KIND_F32, fam_equal, 16384, 9, (2, 2047)),
    ("low_byte", KIND_I64, fam_low_byte, 16384, 9, (2, 255, 2048)),
    ("low_byte", KIND_U32, fam_low_byte, 257, 3, (1, 256)),
    ("two_values", KIND_I64, fam_two_values, 16384, 3, (2048,)),
    ("two_values", KIND_I64, fam_two_values, 16384, 3, (257,)),
    ("ascending", KIND_I64, fam_ascending, 257, 3, (1, 2, 256)),
    ("f32_special", KIND_F32, fam_f32_special, 257, 3, (1, 2, 255, 257, 2048)),
    ("f32_special", KIND_F32, fam_f32_special, 16384, 9, (256, 2047)),
    ("f32_copies", KIND_F32, fam_f32_copies, 16384, 3, (2047,)),
    ("f32_copies", KIND_F32, fam_f32_copies, 16384, 3, (256,)),
    # two levels (16385 .. 4,194,304): group maxima, a dense select over them, a select over the children of its k best with a floor
    ("full", KIND_I64, fam_full, TWO_LEVELS, 3, (1, 2, 256, 2048)),
    ("full", KIND_I64, fam_full, 65537, 9, (255, 257, 2047)),
    ("full", KIND_U32, fam_full, 65537, 3, (1, 2048)),
    ("full", KIND_F32, fam_full, TWO_LEVELS, 3, (2, 2048)),
    ("bands", KIND_I64, fam_bands, TWO_LEVELS, 3, (2, 2048)),
    ("bands", KIND_I64, fam_bands, 65537, 3, (257,)),
    ("equal", KIND_I64, fam_equal, TWO_LEVELS, 3, (1, 255, 2048)),
    ("equal", KIND_U32, fam_equal, 65537, 3, (256,)),
    ("two_values", KIND_I64, fam_two_values, TWO_LEVELS, 3, (2047,)),
    ("two_values", KIND_I64, fam_two_values, 65537, 3, (256,)),
    ("two_values", KIND_I64, fam_two_values, 65537, 3, (2048,)),
    ("low_byte", KIND_I64, fam_low_byte, 65537, 3, (1, 256, 2047)),
    ("low_byte", KIND_U32, fam_low_byte, TWO_LEVELS, 9, (2, 2048)),
    ("ascending", KIND_I64, fam_ascending, TWO_LEVELS, 3, (1, 2, 257, 2048)),
    ("descending", KIND_I64, fam_descending, 65537, 3, (2, 2048)),
    ("one_group", KIND_I64, fam_one_group, 65537, 3, (255,)),
    ("one_group", KIND_I64, fam_one_group, 65537, 3, (256,)),
    ("one_per_group", KIND_I64, fam_one_per_group, 65537, 3, (255,)),
    ("one_per_group", KIND_I64, fam_one_per_group, 65537, 3, (256,)),
    ("shared_group_max", KIND_I64, fam_shared_group_max, 65537, 3, (2,)),
    ("shared_group_max", KIND_I64, fam_shared_group_max, 65537, 3, (255,)),
    ("f32_special", KIND_F32, fam_f32_special, TWO_LEVELS, 3, (2, 257, 2048)),
    ("f32_special", KIND_F32, fam_f32_special, 65537, 9, (1, 2047)),
    ("f32_copies", KIND_F32, fam_f32_copies, TWO_LEVELS, 3, (2048,)),
    ("f32_copies", KIND_F32, fam_f32_copies, 65537, 3, (257,)),
    ("floor_overflow", KIND_I64, fam_floor_overflow, 65537, 3, (255,)),
    ("floor_overflow", KIND_F32, fam_floor_overflow, 65537, 3, (255,)),
    ("full", KIND_I64, fam_full, THREE_LEVELS - 1, 1, (1, 2048)),
    ("ascending", KIND_I64, fam_ascending, THREE_LEVELS - 1, 2, (257,)),
    # three levels (> 4,194,304), nq <= 2
    ("full", KIND_I64, fam_full, THREE_LEVELS, 2, (1, 2, 2048)),
    ("full", KIND_U32, fam_full, THREE_LEVELS + 256, 2, (256,)),
    ("bands", KIND_I64, fam_bands, THREE_LEVELS, 2, (2048,)),
    ("equal", KIND_I64, fam_equal, THREE_LEVELS, 2, (1, 256)),
    ("two_values", KIND_I64, fam_two_values, THREE_LEVELS, 1, (2048,)),
    ("ascending", KIND_I64, fam_ascending, THREE_LEVELS, 1, (2, 257, 2048)),
    ("descending", KIND_I64, fam_descending, THREE_LEVELS + 256, 1, (255,)),
    ("one_per_group", KIND_I64, fam_one_per_group, THREE_LEVELS + 256, 1, (2047,)),
    ("one_per_group", KIND_I64, fam_one_per_group, THREE_LEVELS + 256, 1, (2048,)),
    ("shared_group_max", KIND_I64, fam_shared_group_max, THREE_LEVELS + 256, 1, (2047,)),
    ("f32_special", KIND_F32, fam_f32_special, THREE_LEVELS, 2, (2, 2047)),
]

# element-strided [n][nq_pad] (layout 1: the batched PQ scan's form) and group-major float (layout 2: the matrix-core rounds' form, whose
# levels are built by reduce_max_gq); the padding columns hold the value that would win
LAYOUT_CASES = [
    ("full", KIND_U32, fam_full, 257, 3, 8, 1, (2, 257)),
    ("low_byte", KIND_U32, fam_low_byte, TWO_LEVELS, 9, 16, 1, (256, 2048)),
    ("full", KIND_U32, fam_full, 65537, 3, 4, 1, (2047,)),
    ("bands", KIND_I64, fam_bands, 65537, 3, 5, 1, (1, 257)),
    ("two_values", KIND_I64, fam_two_values, TWO_LEVELS, 9, 10, 1, (255,)),
    ("f32_special", KIND_F32, fam_f32_special, 257, 9, 32, 1, (2, 256)),
    ("f32_special", KIND_F32, fam_f32_special, 257, 9, 32, 2, (1, 255, 2048)),
    ("f32_special", KIND_F32, fam_f32_special, TWO_LEVELS, 3, 4, 2, (2, 2048)),
    ("f32_copies", KIND_F32, fam_f32_copies, TWO_LEVELS, 9, 128, 2, (2047,)),
    ("f32_special", KIND_F32, fam_f32_special, 65537, 9, 32, 2, (257,)),
    ("floor_overflow", KIND_F32, fam_floor_overflow, 65537, 3, 32, 2, (255,)),
    ("equal", KIND_F32, fam_equal, 65537, 3, 5, 2, (256,)),
]


def make_keys(name, kind, fam, n, nq, ks):
    rng = np.random.default_rng(zlib.crc32(f"{name}/{kind}/{n}/{nq}/{ks}".encode()))
    keys = np.ascontiguousarray(fam(rng, kind, nq, n, max(ks)), DT[kind])
    assert keys.shape == (nq, n)
    return keys


# ---- the reference against Python's own sort (no GPU) --------------------------------------------------------------------------------

def python_order(row, kind, k):
    if kind == KIND_F32:   # total order: by value, then +0.0 ahead of -0.0 (the only two floats that compare equal), then by id
        return sorted(range(len(row)), key=lambda i: (-float(row[i]), math.copysign(1.0, float(row[i])) < 0, i))[:k]
    return sorted(range(len(row)), key=lambda i: (-int(row[i]), i))[:k]


@pytest.mark.parametrize("name,kind,fam,k", [
    ("full", KIND_I64, fam_full, 40), ("full", KIND_U32, fam_full, 40), ("bands", KIND_I64, fam_bands, 7), ("equal", KIND_I64, fam_equal, 300),
    ("two_values", KIND_I64, fam_two_values, 100), ("low_byte", KIND_I64, fam_low_byte, 64), ("low_byte", KIND_U32, fam_low_byte, 64),
    ("f32_special", KIND_F32, fam_f32_special, 200), ("equal", KIND_F32, fam_equal, 5), ("full", KIND_F32, fam_full, 90)])
def test_reference_agrees_with_pythons_sort(name, kind, fam, k):
    keys = make_keys(name, kind, fam, 300, 4, (k,))
    for q in range(4):
        assert reference_order(keys[q], kind, k).tolist() == python_order(keys[q], kind, k), (name, q)
        u = sortable(keys[q], kind)                      # the unsigned image orders exactly as the keys do
        o = python_order(keys[q], kind, 300)
        assert all(int(u[a]) >= int(u[b]) for a, b in zip(o, o[1:]))


def merge_inputs(rng, G, nq, k):
    """name -> ([G][nq][k] scores, [G][nq][k] ids): what a gather of G shards' records can hold.  ids are distinct and span the u32 range."""
    total = G * nq * k
    ids0 = (rng.permutation(total).astype(np.uint64) * np.uint64((2 ** 32 - 2) // total) + np.uint64(rng.integers(0, (2 ** 32 - 2) // total))).astype(np.uint32).reshape(G, nq, k)
    full = plant(rng.integers(I64_MIN, I64_MAX, size=(G * nq, k), dtype=np.int64, endpoint=True).reshape(1, -1), [I64_MIN, I64_MAX, I64_MIN, I64_MAX]).reshape(G, nq, k)
    out = {"full_range": (full, ids0)}
    ids = ids0.copy()                                   # whole shards of ID_NONE (every shard when there is one); their scores would win
    sc = full.copy()
    for g in sorted({0, G // 2, G - 1} if G > 3 else {G // 2}):
        ids[g] = ID_NONE
        sc[g] = I64_MAX
    out["empty_shards"] = (sc, ids)
    ids = ids0.copy()                                   # valid ids carrying INT64_MIN next to empty slots (INT64_MIN, ID_NONE)
    sc = np.where(rng.random((G, nq, k)) < 0.9, I64_MIN, full)
    ids[:, :, (k + 1) // 2:] = ID_NONE
    sc[:, :, (k + 1) // 2:] = I64_MIN
    out["saturated_beside_empty"] = (sc, ids)
    out["one_score"] = (np.full((G, nq, k), 12345, np.int64), ids0)
    return out


def by_query(a):
    G, nq, k = a.shape
    return np.ascontiguousarray(a.transpose(1, 0, 2).reshape(nq, G * k))


@pytest.mark.parametrize("G,nq,k", [(1, 1, 1), (3, 4, 10), (8, 3, 64)])
def test_host_merge_orders_by_score_then_id_and_drops_empty_records(mse, G, nq, k):
    """shard.merge_topk_numpy -- the reference of the device merges below -- against this file's own reference, on the same inputs.
    (It used to rank a valid record carrying INT64_MIN FIRST: it sorted by the negated score, and -INT64_MIN wraps.)"""
    from mse import shard
    for name, (sc, ids) in merge_inputs(np.random.default_rng(G * 1000 + k), G, nq, k).items():
        s, i = by_query(sc), by_query(ids)
        want_s, want_i = merge_reference(s, i, k)
        for q in range(nq):     # the reference itself, against Python's sort
            valid = [j for j in range(G * k) if int(i[q, j]) != ID_NONE]
            o = sorted(valid, key=lambda j: (-int(s[q, j]), int(i[q, j])))[:k]
            assert want_i[q, :len(o)].tolist() == [int(i[q, j]) for j in o] and want_s[q, :len(o)].tolist() == [int(s[q, j]) for j in o]
            assert np.all(want_i[q, len(o):] == ID_NONE) and np.all(want_s[q, len(o):] == I64_MIN)
        got_s, got_i = shard.merge_topk_numpy(s, i, k)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s), name


# ---- the device ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sel(gpu, mse):
    s = mse.Searcher(mse.VectorList.generate(SEED_BASE, 0, 64))    # the tournament uses the searcher's scratch and stream only
    yield s
    s.close()


def select_topk(sel, dev_keys, kind, layout, n, nq, nq_pad, k):
    from mse import ffi
    ids = np.full((nq, k), 0xDEADBEEF, np.uint32)
    dt = DT.get(kind, np.int64)
    keys = np.full((nq, k * np.dtype(dt).itemsize), 0x5A, np.uint8).view(dt)
    kth = np.full(nq, 0xA5A5A5A5A5A5A5A5, np.uint64)
    ffi.check(ffi.lib().mse_debug_select_topk(sel._h, kind, layout, dev_keys.ctypes.data, n, nq, nq_pad, k, ids.ctypes.data_as(ffi.u32p),
                                              keys.ctypes.data, kth.ctypes.data_as(C.POINTER(C.c_uint64))), "mse_debug_select_topk")
    return ids, keys, kth


def check_select(sel, keys, kind, ks, layout=0, nq_pad=0):
    nq, n = keys.shape
    ku = sortable(keys, kind)
    order = np.stack([reference_order(keys[q], kind, KMAX) for q in range(nq)])     # computed once, shared by every k
    if layout == 0:
        dev_keys = keys
    else:
        dev_keys = np.full((n, nq_pad), WINNING_PAD[kind], DT[kind])
        dev_keys[:, :nq] = keys.T
    for k in ks:
        m = min(k, n)
        want_ids = np.full((nq, k), ID_NONE, np.uint32)
        want_ids[:, :m] = order[:, :m]
        want_keys = np.full((nq, k), PAD_KEY[kind], DT[kind])
        want_keys[:, :m] = np.take_along_axis(keys, order[:, :m], 1)
        got_ids, got_keys, kth = select_topk(sel, dev_keys, kind, layout, n, nq, nq_pad, k)
        bad = np.argwhere(got_ids != want_ids)
        assert bad.size == 0, f"k={k}: {len(bad)} ids differ, first at (query, rank) {bad[0].tolist()}: got {got_ids[tuple(bad[0])]}, want {want_ids[tuple(bad[0])]}"
        assert np.array_equal(got_keys.view(BITS[kind]), want_keys.view(BITS[kind])), f"k={k}: keys differ"
        if n < k:
            assert not kth.any(), f"k={k} > n={n}: last_kth {kth.tolist()}"
        else:
            kth_true = kth_domain(np.take_along_axis(ku, order[:, k - 1:k], 1)[:, 0], kind)
            assert np.all(kth <= kth_true), f"k={k}: last_kth {kth.tolist()} above the k-th key {kth_true.tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,fam,n,nq,ks", CASES, ids=[f"{c[0]}-kind{c[1]}-n{c[3]}-nq{c[4]}-k{'_'.join(map(str, c[5]))}" for c in CASES])
def test_select_matches_reference(sel, name, kind, fam, n, nq, ks):
    check_select(sel, make_keys(name, kind, fam, n, nq, ks), kind, ks)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,fam,n,nq,nq_pad,layout,ks", LAYOUT_CASES,
                         ids=[f"layout{c[6]}-{c[0]}-kind{c[1]}-n{c[3]}-nq{c[4]}of{c[5]}-k{'_'.join(map(str, c[7]))}" for c in LAYOUT_CASES])
def test_select_strided_layouts_match_reference(sel, name, kind, fam, n, nq, nq_pad, layout, ks):
    check_select(sel, make_keys(name, kind, fam, n, nq, ks), kind, ks, layout, nq_pad)


@pytest.mark.gpu
def test_select_hook_refuses_what_it_does_not_support(sel, mse):
    keys = np.zeros((4, 8), np.int64)                   # large enough for every shape below; nothing is read before the refusal
    for kind, layout, nq_pad, k in [(KIND_I64, 0, 0, 0), (KIND_I64, 0, 0, KMAX + 1), (2, 0, 0, 1), (7, 0, 0, 1), (KIND_I64, 2, 4, 1),
                                    (KIND_U32, 2, 4, 1), (KIND_F32, 3, 4, 1), (KIND_F32, 2, 1, 1), (KIND_U32, 1, 1, 1)]:
        with pytest.raises(mse.MseError, match="select_topk"):
            select_topk(sel, keys, kind, layout, 4, 2, nq_pad, k)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 33])
@pytest.mark.parametrize("k", [1, 10, 1024, 2048])
@pytest.mark.parametrize("G", [1, 3, 8])
def test_device_merges_match_host_merge(sel, mse, G, k, nq):
    """mse_merge_topk_dev ([G][nq][k] arrays) and mse_merge_topk_packed_dev (G packed blocks) against shard.merge_topk_numpy, which the
    CPU test above holds to (score descending, id ascending, ID_NONE absent).  8 x 2048 = 16384 records outgrow the select's LDS list."""
    import torch
    from mse import ffi, shard
    L = ffi.lib()
    B = int(L.mse_topk_block_bytes(nq, k))
    out_s = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    out_i = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    for name, (sc, ids) in merge_inputs(np.random.default_rng(G * 10000 + k * 2 + nq), G, nq, k).items():
        want_s, want_i = shard.merge_topk_numpy(by_query(sc), by_query(ids), k)
        if name == "saturated_beside_empty":            # the saturated valid records are returned, ahead of the empty slots
            n_valid = G * ((k + 1) // 2)
            assert np.all(want_i[:, :min(k, n_valid)] != ID_NONE) and np.all(want_i[:, n_valid:] == ID_NONE)
            if n_valid <= k:                             # ... all of them when no more than k records are valid
                all_i = by_query(ids)
                assert np.array_equal(np.sort(want_i[:, :n_valid], 1), np.sort(all_i[all_i != ID_NONE].reshape(nq, n_valid), 1))
        blocks = np.zeros((G, B), np.uint8)
        blocks[:, :nq * k * 8] = sc.reshape(G, -1).view(np.uint8)
        blocks[:, nq * k * 8:nq * k * 12] = ids.reshape(G, -1).view(np.uint8)
        sd, idd, bd = torch.from_numpy(sc).cuda(), torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(blocks).cuda()
        for form in ("arrays", "packed"):
            out_s.fill_(-7)
            out_i.fill_(-7)
            torch.cuda.synchronize()
            if form == "arrays":
                ffi.check(L.mse_merge_topk_dev(sel._h, sd.data_ptr(), idd.data_ptr(), G, nq, k, out_s.data_ptr(), out_i.data_ptr()))
            else:
                ffi.check(L.mse_merge_topk_packed_dev(sel._h, bd.data_ptr(), G, nq, k, out_s.data_ptr(), out_i.data_ptr()))
            ffi.check(L.mse_device_synchronize())
            assert np.array_equal(out_i.cpu().numpy().view(np.uint32), want_i), (name, form)
            assert np.array_equal(out_s.cpu().numpy(), want_s), (name, form)
