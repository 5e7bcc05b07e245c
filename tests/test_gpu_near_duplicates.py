"""The near-duplicate join on the device (mse_join_self, Searcher.near_duplicates) and the keep-first rule over its pair list, against
the restatement of tests/near_duplicate_ref.py: the oracle's all-pairs scores with band, filter and threshold applied, and a plain Python
walk.  Every comparison of pairs, scores, masks and labels is an equality.  Bases are f16 unit rows from a seeded generator with planted
pairs; random rows score far below the 0.9 threshold, so the planted structure is what the join has to find."""
import numpy as np
import pytest

import near_duplicate_ref as ref
from test_gpu_filtered_graph import clustered_rows

pytestmark = pytest.mark.gpu
TILE = 128            # the kernel's tile height (csrc/kernels.h JOIN_TILE)
NONE = ref.NONE
MODES = ("MODE_EXACT", "MODE_MFMA", "MODE_AUTO")


def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def plant(x, pairs, seed=1, noise=0.15):
    """row hi = row lo + noise, normalised (a score of about 0.99); noise None: a bit-identical copy"""
    rng = np.random.default_rng(seed)
    for lo, hi in pairs:
        if noise is None:
            x[hi] = x[lo]
        else:
            v = x[lo] + noise * rng.standard_normal(x.shape[1]) / np.sqrt(x.shape[1])
            x[hi] = v / np.linalg.norm(v)
    return x


def edge_pairs(n):
    """the placements of the parity test that fit into n rows"""
    p = []
    if n > 70:
        p.append((3, 70))                    # inside a diagonal tile, across its 32-row blocks and its waves
    if n > 9:
        p.append((5, 9))                     # inside one 32-row MFMA block
    if n > TILE:
        p.append((TILE - 1, TILE))           # lo the last row of a tile, hi the first of the next
    if n > 40:
        p.append((0, 40))                    # lo = 0
    if n >= 2:
        p.append((max(0, n - 1 - 200) if n > 2 else 0, n - 1))   # hi = n - 1 in the partial last tile
    return p


class World:
    def __init__(self, mse, orc, x, d):
        self.base = orc.f16_bits(np.asarray(x, np.float32)) if x.dtype != np.uint16 else x
        self.n, self.d = self.base.shape[0], d
        self.S = ref.score_matrix(orc, self.base)
        self.vecs = mse.VectorList.from_f16s(self.base, d)
        self.s = mse.Searcher(self.vecs)

    def want(self, thr, window=0, within=None):
        return ref.pairs_from_scores(self.S, thr, window, within)

    def close(self):
        self.s.close()
        self.vecs.close()


def same_pairs(p, want, tag=None):
    lo, hi, sc = p.read()
    assert p.count == want[0].size, (tag, p.count, want[0].size)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and sc.dtype == np.int64
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]) and np.array_equal(sc, want[2]), tag
    assert not (lo == hi).any(), tag
    return lo, hi, sc


# ---- 1. parity at the tile edges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 192, 1152])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_parity_at_tile_edges(gpu, mse, orc, n, d):
    x = plant(unit_rows(n, d, 100 + n), edge_pairs(n), noise=0.1)
    if n > 21:
        plant(x, [(11, 21)], noise=None)     # bit-identical rows
    w = World(mse, orc, x, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert want[0].size >= len(edge_pairs(n)), "the planted pairs must be pairs of the restatement"
    assert (np.diag(w.S) >= thr).all(), "every row scores about 1 against itself"
    for mode in MODES:
        p = w.s.near_duplicates(thr, mode=getattr(mse, mode))
        assert len(p) == n
        same_pairs(p, want, mode)
        assert w.s.join_stats()["kept"] == want[0].size
        p.close()
    # the part reads of the canonical order
    if want[0].size >= 2:
        p = w.s.near_duplicates(0.9)          # a float threshold goes through scale_dot_result
        lo, hi, sc = p.read(1, 1)
        assert (lo[0], hi[0], sc[0]) == (want[0][1], want[1][1], want[2][1])
        with pytest.raises(mse.MseError):
            p.read(1, want[0].size)
        p.close()
    w.close()


# ---- 2. the threshold is exact -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 1152])
def test_threshold_is_exact(gpu, mse, orc, d):
    n = TILE + 40
    w = World(mse, orc, plant(unit_rows(n, d, 7), [(17, TILE + 3)]), d)
    s = int(w.S[TILE + 3, 17])
    assert s == int(w.S[17, TILE + 3]) and s > mse.scale_dot_result(0.9)
    for mode in MODES:
        p = w.s.near_duplicates(s, mode=getattr(mse, mode))
        lo, hi, sc = same_pairs(p, w.want(s), mode)
        assert (lo.tolist(), hi.tolist(), sc.tolist()) == ([17], [TILE + 3], [s])
        p.close()
        p = w.s.near_duplicates(s + 1, mode=getattr(mse, mode))
        assert p.count == 0
        st = w.s.join_stats()
        p.close()
        if mode != "MODE_EXACT":   # nominated by the matrix cores, rejected by the re-score
            assert st["nominated"] >= 1 and st["rescored"] == st["nominated"] and st["kept"] == 0, st
    w.close()


# ---- 3. the filter filters, and a full candidate buffer changes nothing ---------------------------------------------------------------

def test_nomination_is_tight_and_capacity_free(gpu, mse, orc):
    n, d = 3 * TILE + 5, 1152
    x = plant(unit_rows(n, d, 9), edge_pairs(n) + [(200, 300), (201, 300), (202, 300), (300, 380)])
    w = World(mse, orc, x, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    p = w.s.near_duplicates(thr, mode=mse.MODE_MFMA)
    ref_bytes = [a.tobytes() for a in same_pairs(p, want)]
    st = w.s.join_stats()
    p.close()
    # the allowance of the certificate from the base's norms, and the pairs whose float64 product lies within twice of it
    f = orc.f16_to_f32(w.base).astype(np.float64)
    bound = 2.8e-4 * float(np.linalg.norm(f, axis=1).max()) ** 2
    g = f @ f.T
    near = int((np.tril(g, -1) >= 0.9 - 2 * bound)[np.tril_indices(n, -1)].sum())
    print("kept", st["kept"], "nominated", st["nominated"], "within 2 bound", near, "tiles", st["tiles"])
    assert st["kept"] == want[0].size and st["kept"] <= st["nominated"] <= near, (st, near)
    assert st["strips_repeated"] == 0 and st["tiles"] == 4 * 5 // 2
    for cap in (1, 3):
        w.s.debug_join_candidate_capacity(cap)
        p = w.s.near_duplicates(thr, mode=mse.MODE_MFMA)
        assert [a.tobytes() for a in same_pairs(p, want, cap)] == ref_bytes
        st2 = w.s.join_stats()
        assert st2["strips_repeated"] >= (st["nominated"] + cap - 1) // cap and st2["nominated"] == st["nominated"], (cap, st2)
        p.close()
        p = w.s.near_duplicates(thr, mode=mse.MODE_EXACT)
        assert [a.tobytes() for a in same_pairs(p, want, ("exact", cap))] == ref_bytes and w.s.join_stats()["strips_repeated"] > 0
        p.close()
    w.s.debug_join_candidate_capacity(0)
    w.close()


# ---- 4. subnormal and mixed-magnitude rows; a non-finite component -------------------------------------------------------------------

def test_subnormal_rows_and_non_finite_component(gpu, mse, orc):
    n, d = TILE + 70, 192
    x = unit_rows(n, d, 21)
    sub = [4, 60, 130, 150]
    for r in sub:                              # half of the components go into the f16 subnormal range (below 6.1e-5)
        x[r, d // 2:] *= 2.0 ** -12
        x[r, :d // 2] /= np.linalg.norm(x[r, :d // 2])
    plant(x, [(4, 61), (60, 131), (130, 151), (20, 100)], noise=0.05)
    plant(x, [(150, 160)], noise=None)
    base = orc.f16_bits(x.astype(np.float32))
    f = orc.f16_to_f32(base)
    assert ((np.abs(f[sub]) < 6.1e-5) & (f[sub] != 0)).sum() > d // 4, "the rows must hold subnormal components"
    w = World(mse, orc, base, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert want[0].size >= 5
    for mode in MODES:
        p = w.s.near_duplicates(thr, mode=getattr(mse, mode))
        same_pairs(p, want, mode)
        p.close()
    st = w.s.join_stats()
    assert st["nominated"] >= st["kept"] == want[0].size
    w.close()
    # one infinite and one NaN component: no bound can be stated, the exact path runs whatever the mode asks for
    base2 = base.copy()
    base2[33, 5] = 0x7C00
    base2[90, 7] = 0x7E00
    w = World(mse, orc, base2, d)
    want = w.want(thr)
    for mode in MODES:
        p = w.s.near_duplicates(thr, mode=getattr(mse, mode))
        same_pairs(p, want, mode)
        st = w.s.join_stats()
        assert st["nominated"] == st["kept"] == want[0].size, (mode, st)   # the exact tiles nominate what they confirm
        p.close()
    w.close()


# ---- 5. window and within ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def band_world(gpu, mse, orc):
    n, d = 3 * TILE + 5, 192
    # distances 1, 2, TILE - 1, TILE, TILE + 1, TILE + 2 and one longer than any window below
    pairs = [(10, 11), (20, 22), (30, 30 + TILE - 1), (40, 40 + TILE), (50, 50 + TILE + 1), (60, 60 + TILE + 2), (2, 380)]
    return World(mse, orc, plant(unit_rows(n, d, 31), pairs), d)


@pytest.mark.parametrize("window", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 50])
def test_window(band_world, mse, window):
    w = band_world
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr, window)
    assert want[0].size >= 1 and (window > w.n or want[0].size < w.want(thr)[0].size)
    dist = (want[1] - want[0]).tolist()
    assert window > w.n or (window in dist and window + 1 not in dist)
    for mode in MODES:
        p = w.s.near_duplicates(thr, window=window, mode=getattr(mse, mode))
        same_pairs(p, want, (window, mode))
        p.close()


def test_within(band_world, mse):
    w = band_world
    thr = mse.scale_dot_result(0.9)
    p = w.s.near_duplicates(thr, mode=mse.MODE_MFMA)
    all_tiles = w.s.join_stats()["tiles"]
    p.close()
    assert all_tiles == 4 * 5 // 2
    one = np.ones(w.n, bool)
    one[40] = False                                  # one row of the pair (40, 40 + TILE)
    tiles = np.ones(w.n, bool)
    tiles[:2 * TILE] = False                         # two whole tiles
    cases = {"one row": (one, None), "whole tiles": (tiles, 3), "nothing": (np.zeros(w.n, bool), 0), "short": (np.ones(200, bool), 3)}
    for name, (mask, n_tiles) in cases.items():
        f = mse.RowFilter(mask)
        want = w.want(thr, 0, mask)
        for mode in MODES:
            p = w.s.near_duplicates(thr, within=f, mode=getattr(mse, mode))
            same_pairs(p, want, (name, mode))
            if n_tiles is not None:
                assert w.s.join_stats()["tiles"] == n_tiles < all_tiles, (name, mode, w.s.join_stats())
            kept, rep = ref.keep_first(w.n, want[0], want[1])
            d = p.duplicates()
            assert np.array_equal(d.to_mask(), ~kept), (name, mode)
            d.close()
            p.close()
        f.close()
    assert w.want(thr, 0, one)[0].size == w.want(thr)[0].size - 1
    assert w.want(thr, 0, np.zeros(w.n, bool))[0].size == 0


# ---- 6. keep-first ------------------------------------------------------------------------------------------------------------------------

def gram_rows(k, edges, d):
    """k unit rows with dot 0.925 along `edges` and 0.85 elsewhere (a factor of the Gram matrix; exact up to the f16 rounding, which is far
    inside the 0.025 margins around the 0.9 threshold)"""
    g = np.full((k, k), 0.85)
    for a, b in edges:
        g[a, b] = g[b, a] = 0.925
    np.fill_diagonal(g, 1.0)
    lam, v = np.linalg.eigh(g)
    assert lam.min() > -1e-9, "the wanted Gram matrix must be positive semi-definite"
    x = np.zeros((k, d))
    x[:, :k] = v * np.sqrt(np.clip(lam, 0, None))
    return x


def path_rows(m, d):
    """x_i = c e_0 + s (e_{i+1} + e_{i+2}) / sqrt 2 with c^2 = 0.85: neighbours score 0.925, all other pairs 0.85"""
    c, s = np.sqrt(0.85), np.sqrt(0.15)
    x = np.zeros((m, d))
    x[:, 0] = c
    for i in range(m):
        x[i, i + 1] = x[i, i + 2] = s / np.sqrt(2)
    return x


SHAPES = {
    "triangle": (3, [(0, 1), (1, 2)]),
    "star, centre first": (4, [(0, 1), (0, 2), (0, 3)]),
    "star, centre last": (4, [(0, 3), (1, 3), (2, 3)]),
    "two overlapping stars": (8, [(0, 1), (0, 2), (0, 3), (3, 5), (5, 6), (5, 7)]),
    "lowest kept neighbour": (5, [(0, 1), (1, 4), (2, 4), (3, 4)]),
}


@pytest.mark.parametrize("shape", list(SHAPES) + ["path"])
def test_keep_first(gpu, mse, orc, shape):
    if shape == "path":
        d, k = 1152, 300
        x = path_rows(k, d)
        edges = [(i, i + 1) for i in range(k - 1)]
    else:
        d = 64
        k, edges = SHAPES[shape]
        x = gram_rows(k, edges, d)
    w = World(mse, orc, x, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert sorted(zip(want[0].tolist(), want[1].tolist())) == sorted(edges), "the base must realise the wanted pair graph"
    kept, rep = ref.keep_first(k, want[0], want[1])
    lab = ref.labels(kept, rep)
    out = []
    for run in range(2):
        p = w.s.near_duplicates(thr, mode=mse.MODE_MFMA if run else mse.MODE_AUTO)
        same_pairs(p, want, shape)
        dup, grp, reps = p.duplicates(), p.groups(), p.representatives()
        assert len(dup) == k and np.array_equal(dup.to_mask(), ~kept) and dup.count == int((~kept).sum())
        assert reps.dtype == np.uint32 and np.array_equal(reps, rep)
        assert len(grp) == k and np.array_equal(grp.to_host(), lab)
        sc = w.S[np.arange(k), rep]
        assert (sc[~kept] >= thr).all(), "every member scores at least the threshold against its representative"
        st = w.s.join_stats()
        out.append((dup.to_mask().tobytes(), reps.tobytes(), grp.to_host().tobytes(), st["rounds"]))
        dup.close()
        grp.close()
        p.close()
    assert out[0] == out[1], "two runs give the same bytes"
    if shape == "path":
        assert kept.tolist() == [i % 2 == 0 for i in range(k)] and out[0][3] > 1
    if shape == "triangle":
        assert kept.tolist() == [True, False, True]
    w.close()


# ---- 7. the values plug in --------------------------------------------------------------------------------------------------------------

def test_values_plug_into_the_index(gpu, mse, orc):
    n, d, k = 3000, 1152, 10
    x = clustered_rows(orc, n, d, n_centres=50, noise=0.5, seed=17).astype(np.float64)
    rng = np.random.default_rng(3)
    heads = rng.choice(n // 2, 40, replace=False)
    planted = []
    for h in heads:                                   # clusters of 2 .. 4 near-copies, scattered over the later rows
        for m in rng.choice(np.arange(n // 2, n), rng.integers(1, 4), replace=False):
            planted.append((int(h), int(m)))
    plant(x, planted, noise=0.1)
    w = World(mse, orc, x, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    kept, rep = ref.keep_first(n, want[0], want[1])
    lab = ref.labels(kept, rep)
    assert (~kept).sum() >= 40
    pairs = w.s.near_duplicates(thr)
    same_pairs(pairs, want)
    # grouped brute force == the numpy collapse of the oracle's ranking under the restated labels
    q = orc.f16_bits(x[heads[:6]].astype(np.float32))
    grp = pairs.groups()
    got_s, got_i = w.s.bruteforce_topk(q, k, groups=grp)
    for qi in range(len(q)):
        sc = orc.score_all(w.base, q[qi])
        order = sorted(range(n), key=lambda r: (-int(sc[r]), r))
        seen, ids = set(), []
        for r in order:
            key = ("g", int(lab[r])) if lab[r] != NONE else ("r", r)
            if key not in seen:
                seen.add(key)
                ids.append(r)
            if len(ids) == k:
                break
        assert np.array_equal(got_i[qi], np.array(ids, np.uint32)) and np.array_equal(got_s[qi], sc[ids]), qi
    grp.close()
    # delete the duplicates from a graph index; a search afterwards returns no dropped row
    g = mse.BuildGraph(n, 32)
    g.random_fill(9)
    med = mse.medioid(w.vecs)
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    g.build(w.s, np.random.default_rng(9).permutation(n).astype(np.uint32), med, cfg, 1024)
    dup = pairs.duplicates()
    if not kept[med]:
        med = int(rep[med])
    st = g.delete_rows(w.s, dup, cfg)
    assert st["deleted"] == int((~kept).sum())
    for ids, _, _ in g.search_batch(w.s, med, q, 48):
        assert kept[ids].all()
    # the graph's own join: a deleted member of a planted pair no longer pairs
    again = g.near_duplicates(w.s, thr)
    assert again.count == 0, "the kept rows are an independent set of the pair graph"
    again.close()
    h = g.to_host()
    dg = mse.DeviceGraph(mse.IndexGraph(h.adj, h.deg))
    full = dg.near_duplicates(w.s, thr)
    same_pairs(full, want)                            # a graph that was never deleted from: every row is live
    full.close()
    lo0, hi0 = int(want[0][0]), int(want[1][0])
    gone = np.zeros(n, bool)
    gone[hi0] = True
    dg.delete_rows(w.s, gone, cfg)
    less = dg.near_duplicates(w.s, thr)
    same_pairs(less, w.want(thr, 0, ~gone))
    lo, hi, _ = less.read()
    assert not ((lo == lo0) & (hi == hi0)).any() and not (hi == hi0).any() and not (lo == hi0).any()
    less.close()
    dg.close()
    dup.close()
    g.close()
    pairs.close()
    w.close()


# ---- 8. errors and overflow --------------------------------------------------------------------------------------------------------------

def test_errors_and_overflow(gpu, mse, orc):
    n, d = TILE + 9, 64
    x = plant(unit_rows(n, d, 5), [(1, 2), (3, 130), (4, 131)], noise=0.05)
    w = World(mse, orc, x, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert want[0].size >= 3
    for mode in MODES:
        with pytest.raises(mse.MseError, match="max_pairs"):
            w.s.near_duplicates(thr, mode=getattr(mse, mode), max_pairs=want[0].size - 1)
        assert w.s.join_stats()["kept"] == want[0].size            # the true count, so the caller can ask again
        p = w.s.near_duplicates(thr, mode=getattr(mse, mode), max_pairs=want[0].size)   # the searcher answers as a fresh one
        same_pairs(p, want, mode)
        p.close()
    long = mse.RowFilter(np.ones(n + 1, bool))
    with pytest.raises(mse.MseError, match="filter is longer than the base"):
        w.s.near_duplicates(thr, within=long)
    long.close()
    with pytest.raises(mse.MseError, match="unknown mode"):
        w.s.near_duplicates(thr, mode=7)
    if gpu >= 2:
        from mse import ffi
        ffi.check(ffi.lib().mse_set_device(1))
        other = mse.RowFilter(np.ones(n, bool))
        ffi.check(ffi.lib().mse_set_device(0))
        with pytest.raises(mse.MseError, match="another device"):
            w.s.near_duplicates(thr, within=other)
        other.close()
    with pytest.raises(TypeError):
        w.s.near_duplicates(thr, within=np.ones(n, bool))
    p = w.s.near_duplicates(thr)
    same_pairs(p, want, "after the errors")
    p.close()
    w.close()
    # no rows: an empty list, and its duplicates() and groups() are empty
    empty = mse.VectorList.from_f16s(np.zeros((0, 64), np.uint16), 64)
    s0 = mse.Searcher(empty)
    p = s0.near_duplicates(thr)
    assert len(p) == 0 and p.count == 0 and p.read()[0].size == 0
    dup, grp = p.duplicates(), p.groups()
    assert len(dup) == 0 and dup.count == 0 and len(grp) == 0 and p.representatives().size == 0
    dup.close()
    grp.close()
    p.close()
    s0.close()
    empty.close()
