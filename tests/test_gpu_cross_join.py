"""The cross join on the device (mse_join_cross, Searcher.near_duplicates_of), admission (mse_pairs_admit), the select of the admitted
rows (mse_base_select) and DeviceGraph.insert_unique_rows, against the restatement of tests/cross_join_ref.py: the oracle's score of every
base row against each incoming row with filter and threshold applied, and a plain Python walk.  Every comparison of pairs, scores, masks
and representatives is an equality.  Bases are f16 unit rows from a seeded generator with planted pairs; random rows score far below the
0.9 threshold, so the planted structure is what the join has to find."""
import numpy as np
import pytest

import cross_join_ref as ref
import near_duplicate_ref as self_ref
from conftest import make_pq
from test_gpu_filtered_graph import clustered_rows
from test_gpu_near_duplicates import unit_rows, plant, TILE, MODES

pytestmark = pytest.mark.gpu
NONE = ref.NONE


def bits(orc, x):
    x = np.asarray(x)
    return np.ascontiguousarray(x) if x.dtype == np.uint16 else orc.f16_bits(x.astype(np.float32))


def plant_cross(xb, xq, pairs, seed=1, noise=0.1, into="incoming"):
    """pairs of (base row, incoming row): the incoming row becomes the base row + noise, normalised (into="base": the other way round);
    noise None: a bit-identical copy"""
    n = len(xb)
    z = np.vstack([xb, xq])
    plant(z, [(b, n + j) if into == "incoming" else (n + j, b) for b, j in pairs], seed, noise)
    xb[:], xq[:] = z[:n], z[n:]


class World:
    """a resident base with its searcher, an incoming base, and the restatement of their cross list"""

    def __init__(self, mse, orc, xb, xq, d):
        self.mse, self.orc, self.d = mse, orc, d
        self.base, self.inc = bits(orc, xb).reshape(-1, d), bits(orc, xq).reshape(-1, d)
        self.n, self.m = self.base.shape[0], self.inc.shape[0]
        self.vecs = mse.VectorList.from_f16s(self.base, d)
        self.s = mse.Searcher(self.vecs)
        self.q = mse.VectorList.from_f16s(self.inc, d)

    def want(self, thr, within=None, rows=None):
        inc = self.inc if rows is None else self.inc[rows[0]:rows[1]]
        return ref.cross_pairs(self.orc, self.base, inc, thr, within)

    def join(self, thr, **kw):
        return self.s.near_duplicates_of(self.q, thr, **kw)

    def close(self):
        self.s.close()
        self.vecs.close()
        self.q.close()


def same_pairs(p, want, tag=None):
    lo, hi, sc = p.read()
    assert p.count == want[0].size, (tag, p.count, want[0].size)
    assert lo.dtype == np.uint32 and hi.dtype == np.uint32 and sc.dtype == np.int64
    assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]) and np.array_equal(sc, want[2]), tag
    return lo, hi, sc


def has_pairs(want, pairs):
    got = set(zip(want[0].tolist(), want[1].tolist()))
    return all((b, j) in got for b, j in pairs)


# ---- 1. parity at the tile edges ---------------------------------------------------------------------------------------------------

def edge_world(mse, orc, n, m, d):
    """the placements of the parity test that fit into n base rows and m incoming rows -> (World, planted (base row, incoming row))"""
    xb, xq = unit_rows(n, d, 100 + n), unit_rows(m, d, 300 + m)
    planted, used = [], set()

    def take(cands):
        out = []
        for b, j in cands:
            if b < n and j < m and j not in used:
                used.add(j)
                out.append((b, j))
        return out
    # one incoming row with three base partners, in different tiles where the base has them: the partners are copies of one another first
    trio = (5, 200, 300) if n > 300 else (5, 50, 100) if n > 100 else None
    if trio and m > 40:
        plant(xb, [(trio[0], trio[1]), (trio[0], trio[2])], seed=2, noise=0.05)
    edges = take([(0, 0), (TILE - 1, TILE), (TILE, TILE - 1), (3, 70), (70, 3), (n - 1, m - 1)])   # (3, 70) and (70, 3): across the 32-row
    plant_cross(xb, xq, edges, noise=0.1)                                                        # blocks and waves, both orientations
    planted += edges
    same = take([(min(11, n - 1), 21), (min(11, n - 1), 1)])[:1]
    plant_cross(xb, xq, same, noise=None)                      # a bit-identical copy
    planted += same
    if trio:
        one = take([(trio[0], 40)])
        plant_cross(xb, xq, one, seed=3, noise=0.05)
        planted += [(b, j) for _, j in one for b in trio]
    fan = take([(9, 6), (9, 140 if m > 250 else 60), (9, 250 if m > 250 else 100)])   # one base row with three incoming partners
    plant_cross(xb, xq, fan, seed=4, noise=0.1)
    planted += fan
    return World(mse, orc, xb, xq, d), planted


@pytest.mark.parametrize("d", [64, 192, 1152])
@pytest.mark.parametrize("n,m", [(1, 1), (127, 129), (128, 128), (129, 127), (389, 1), (1, 259), (389, 259)])
def test_parity_at_tile_edges(gpu, mse, orc, n, m, d):
    w, planted = edge_world(mse, orc, n, m, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert planted and has_pairs(want, planted), "the planted pairs must be pairs of the restatement"
    if n == 389 and m == 259:
        assert len(planted) >= 13 and np.bincount(want[1], minlength=m)[40] >= 3 and (want[0] == 9).sum() >= 3
    for mode in MODES:
        p = w.join(thr, mode=getattr(mse, mode))
        assert len(p) == m and p.kind == 1 and p.base_rows == n
        same_pairs(p, want, mode)
        assert w.s.join_stats()["kept"] == want[0].size
        p.close()
    p = w.join(0.9)                               # a float threshold goes through scale_dot_result
    same_pairs(p, want, "float threshold")
    if want[0].size >= 2:                         # the part reads of the canonical order
        lo, hi, sc = p.read(1, 1)
        assert (lo[0], hi[0], sc[0]) == (want[0][1], want[1][1], want[2][1])
    with pytest.raises(mse.MseError):
        p.read(1, want[0].size)                   # a read past the end
    p.close()
    q = w.s.near_duplicates_of(w.inc, thr)        # a numpy array is uploaded by the wrapper
    same_pairs(q, want, "numpy incoming")
    q.close()
    w.close()


# ---- 2. the threshold is exact -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 1152])
def test_threshold_is_exact(gpu, mse, orc, d):
    n, m = TILE + 40, TILE + 9
    xb, xq = unit_rows(n, d, 7), unit_rows(m, d, 8)
    plant_cross(xb, xq, [(17, TILE + 3)], noise=0.15)
    w = World(mse, orc, xb, xq, d)
    s = int(orc.score_all(w.base, w.inc[TILE + 3])[17])
    assert s > mse.scale_dot_result(0.9)
    for mode in MODES:
        p = w.join(s, mode=getattr(mse, mode))
        lo, hi, sc = same_pairs(p, w.want(s), mode)
        assert (lo.tolist(), hi.tolist(), sc.tolist()) == ([17], [TILE + 3], [s])
        p.close()
        p = w.join(s + 1, mode=getattr(mse, mode))
        assert p.count == 0 and len(p) == m
        st = w.s.join_stats()
        p.close()
        if mode != "MODE_EXACT":   # nominated by the matrix cores, rejected by the re-score
            assert st["nominated"] >= 1 and st["rescored"] == st["nominated"] and st["kept"] == 0, st
    w.close()


# ---- 3. nomination is tight, and a full candidate buffer changes nothing ------------------------------------------------------------

def test_nomination_is_tight_and_capacity_free(gpu, mse, orc):
    n, m, d = 3 * TILE + 5, 2 * TILE + 3, 1152
    w, planted = edge_world(mse, orc, n, m, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert has_pairs(want, planted)
    p = w.join(thr, mode=mse.MODE_MFMA)
    ref_bytes = [a.tobytes() for a in same_pairs(p, want)]
    st = w.s.join_stats()
    p.close()
    # the documented bound for a pair of the two bases: 2.8e-4 x the larger of the two largest row norms, squared (these rows hold too
    # little subnormal mass for the second term to matter inside the factor two); the pairs whose float64 product lies within twice of it
    fb, fq = orc.f16_to_f32(w.base).astype(np.float64), orc.f16_to_f32(w.inc).astype(np.float64)
    bound = 2.8e-4 * max(float(np.linalg.norm(fb, axis=1).max()), float(np.linalg.norm(fq, axis=1).max())) ** 2
    near = int((fq @ fb.T >= 0.9 - 2 * bound).sum())
    print("kept", st["kept"], "nominated", st["nominated"], "within 2 bound", near, "tiles", st["tiles"])
    assert st["kept"] == want[0].size and st["kept"] <= st["nominated"] <= near, (st, near)
    assert st["strips_repeated"] == 0 and st["tiles"] == 4 * 3      # the rectangle's tile count
    for cap in (1, 3):
        w.s.debug_join_candidate_capacity(cap)
        p = w.join(thr, mode=mse.MODE_MFMA)
        assert [a.tobytes() for a in same_pairs(p, want, cap)] == ref_bytes
        st2 = w.s.join_stats()
        assert st2["strips_repeated"] >= (st["nominated"] + cap - 1) // cap and st2["nominated"] == st["nominated"], (cap, st2)
        assert st2["tiles"] == 4 * 3
        p.close()
        p = w.join(thr, mode=mse.MODE_EXACT)
        assert [a.tobytes() for a in same_pairs(p, want, ("exact", cap))] == ref_bytes and w.s.join_stats()["strips_repeated"] > 0
        p.close()
    w.s.debug_join_candidate_capacity(0)
    p = w.join(thr)                                                  # the searcher answers as a fresh one
    assert [a.tobytes() for a in same_pairs(p, want)] == ref_bytes and w.s.join_stats()["strips_repeated"] == 0
    p.close()
    w.close()


# ---- 4. magnitudes and non-finite values -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["incoming", "base"])
def test_subnormal_rows_on_one_side(gpu, mse, orc, side):
    n, m, d = TILE + 70, TILE + 22, 192
    xb, xq = unit_rows(n, d, 21), unit_rows(m, d, 22)
    own, other = (xq, xb) if side == "incoming" else (xb, xq)
    sub = [4, 60, 130]
    for r in sub:                              # half of the components go into the f16 subnormal range (below 6.1e-5)
        own[r, d // 2:] *= 2.0 ** -12
        own[r, :d // 2] /= np.linalg.norm(own[r, :d // 2])
    pairs = [(61, 4), (131, 60), (7, 130)] if side == "incoming" else [(4, 61), (60, 131), (130, 7)]
    plant_cross(xb, xq, pairs, noise=0.05, into="base" if side == "incoming" else "incoming")   # the partners copy the subnormal rows
    plant_cross(xb, xq, [(20, 100)], noise=0.05)
    w = World(mse, orc, xb, xq, d)
    own_bits, other_bits = (w.inc, w.base) if side == "incoming" else (w.base, w.inc)
    f = orc.f16_to_f32(own_bits)
    assert ((np.abs(f[sub]) < 6.1e-5) & (f[sub] != 0)).sum() > d // 4, "the rows must hold subnormal components"
    g = orc.f16_to_f32(other_bits)
    mass = lambda v: np.where(np.abs(v) < 6.1e-5, np.abs(v), 0).sum(axis=1).max()
    assert mass(g) < mass(f) / 10, "the other base's figure alone would not cover the pair"
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert has_pairs(want, pairs + [(20, 100)])
    for mode in MODES:
        p = w.join(thr, mode=getattr(mse, mode))
        same_pairs(p, want, (side, mode))
        p.close()
    st = w.s.join_stats()
    assert st["nominated"] >= st["kept"] == want[0].size
    w.close()


@pytest.mark.parametrize("long_side", ["incoming", "base"])
def test_mixed_magnitudes(gpu, mse, orc, long_side):
    """rows of norm 8 on one side against rows of norm 1/8 on the other: the products are of order 1, the bound must come from the longer
    side.  Near copies (noise 0.1: about 0.995) lie above the threshold 0.9, far copies (noise 0.55: about 0.876) below it."""
    n, m, d = TILE + 70, TILE + 22, 1152
    xb, xq = unit_rows(n, d, 41), unit_rows(m, d, 42)
    above, below = [(3, 5), (TILE + 1, TILE + 2), (100, 20)], [(8, 9), (TILE + 7, 40), (90, TILE + 11)]
    plant_cross(xb, xq, above, noise=0.1)
    plant_cross(xb, xq, below, seed=2, noise=0.55)
    sb, sq = (0.125, 8.0) if long_side == "incoming" else (8.0, 0.125)
    w = World(mse, orc, xb * sb, xq * sq, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    got = set(zip(want[0].tolist(), want[1].tolist()))
    assert all(p in got for p in above) and not any(p in got for p in below), "pairs on both sides of the threshold"
    for mode in MODES:
        p = w.join(thr, mode=getattr(mse, mode))
        same_pairs(p, want, (long_side, mode))
        st = w.s.join_stats()
        assert st["nominated"] >= st["kept"] == want[0].size, (mode, st)
        p.close()
    w.close()


@pytest.mark.parametrize("side", ["incoming", "base"])
def test_non_finite_component(gpu, mse, orc, side):
    """one infinite and one NaN component in one of the bases: no bound can be stated, the exact path runs whatever the mode asks for"""
    n, m, d = TILE + 70, TILE + 22, 192
    xb, xq = unit_rows(n, d, 51), unit_rows(m, d, 52)
    plant_cross(xb, xq, [(4, 61), (130, 7), (20, 100)], noise=0.05)
    b, q = bits(orc, xb), bits(orc, xq)
    bad = q if side == "incoming" else b
    bad[33, 5] = 0x7C00
    bad[90, 7] = 0x7E00
    w = World(mse, orc, b, q, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert has_pairs(want, [(4, 61), (130, 7), (20, 100)])
    for mode in MODES:
        p = w.join(thr, mode=getattr(mse, mode))
        same_pairs(p, want, (side, mode))
        st = w.s.join_stats()
        assert st["nominated"] == st["kept"] == want[0].size, (mode, st)   # the exact tiles nominate what they confirm
        p.close()
    w.close()


# ---- 5. filter, batch cut and presentation -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rect_world(gpu, mse, orc):
    w, planted = edge_world(mse, orc, 3 * TILE + 5, 2 * TILE + 3, 192)
    w.planted = planted
    return w


def test_within(rect_world, mse):
    w = rect_world
    thr = mse.scale_dot_result(0.9)
    p = w.join(thr, mode=mse.MODE_MFMA)
    all_tiles = w.s.join_stats()["tiles"]
    p.close()
    assert all_tiles == 4 * 3
    one = np.ones(w.n, bool)
    one[9] = False                                   # the base row with three incoming partners
    first = np.ones(w.n, bool)
    first[:TILE] = False                             # a whole base tile
    cases = {"one row": (one, None), "a whole base tile": (first, all_tiles - 3), "nothing": (np.zeros(w.n, bool), 0),
             "short": (np.ones(200, bool), 2 * 3)}
    full = w.want(thr)[0].size
    for name, (mask, n_tiles) in cases.items():
        f = mse.RowFilter(mask)
        want = w.want(thr, mask)
        for mode in MODES:
            p = w.join(thr, within=f, mode=getattr(mse, mode))
            same_pairs(p, want, (name, mode))
            assert len(p) == w.m
            if n_tiles is not None:   # a tile whose base rows are all excluded does no work: one per incoming tile
                assert w.s.join_stats()["tiles"] == n_tiles, (name, mode, w.s.join_stats())
            p.close()
        f.close()
    assert w.want(thr, one)[0].size <= full - 3 and w.want(thr, np.zeros(w.n, bool))[0].size == 0
    assert 0 < w.want(thr, np.ones(200, bool))[0].size < full and (w.want(thr, np.ones(200, bool))[0] < 200).all()


@pytest.mark.parametrize("a,c", [(5, 200), (130, 259)])
def test_batch_cut(rect_world, mse, a, c):
    """the list of rows [a, c) of the incoming base, given alone, is the slice of the whole list with hi shifted by a"""
    w = rect_world
    thr = mse.scale_dot_result(0.9)
    whole = w.want(thr)
    sel = (whole[1] >= a) & (whole[1] < c)
    want = (whole[0][sel], (whole[1][sel] - a).astype(np.uint32), whole[2][sel])
    assert want[0].size >= 3 and np.array_equal(np.stack(want[:2]), np.stack(w.want(thr, rows=(a, c))[:2]))
    for mode in MODES:
        p = w.s.near_duplicates_of(w.inc[a:c], thr, mode=getattr(mse, mode))
        assert len(p) == c - a and p.base_rows == w.n
        same_pairs(p, want, (a, c, mode))
        p.close()


def test_host_made_and_wrapped_incoming_give_the_same_bytes(rect_world, mse):
    import torch
    w = rect_world
    thr = mse.scale_dot_result(0.9)
    p = w.join(thr)
    ref_bytes = [x.tobytes() for x in same_pairs(p, w.want(thr))]
    p.close()
    t = torch.from_numpy(w.inc.view(np.int16).copy()).cuda()
    wrapped = mse.VectorList.wrap_device(t.data_ptr(), w.m, w.d, keepalive=t)
    for mode in MODES:
        p = w.s.near_duplicates_of(wrapped, thr, mode=getattr(mse, mode))
        assert [x.tobytes() for x in p.read()] == ref_bytes, mode
        p.close()
    wrapped.close()


# ---- 6. admission -----------------------------------------------------------------------------------------------------------------

def gram_rows(k, edges, d, edge=0.92, rest=0.86):
    """k unit rows with dot `edge` along `edges` and `rest` elsewhere (a factor of the Gram matrix, as the self-join's gram_rows; exact up
    to the f16 rounding, which is far inside the 0.02 margins around the 0.9 threshold).  These constants keep the matrix positive
    semi-definite for every tree whose adjacency spectrum lies above -2.33: a path with pendant rows included."""
    g = np.full((k, k), rest)
    for a, b in edges:
        g[a, b] = g[b, a] = edge
    np.fill_diagonal(g, 1.0)
    lam, v = np.linalg.eigh(g)
    assert lam.min() > -1e-9, "the wanted Gram matrix must be positive semi-definite"
    x = np.zeros((k, d))
    x[:, :k] = v * np.sqrt(np.clip(lam, 0, None))
    return x


# name: (base rows, incoming rows, pairs (base row, incoming row), pairs among the incoming rows)
ADMIT = {
    "chain through a dropped row": (1, 2, [(0, 0)], [(0, 1)]),
    "dropped by the base and by a kept row": (1, 2, [(0, 1)], [(0, 1)]),
    "alternating path, row 0 has base partners": (2, 9, [(0, 0), (1, 0)], [(i, i + 1) for i in range(8)]),
    "lowest kept neighbour": (1, 5, [], [(0, 1), (1, 4), (2, 4), (3, 4)]),
    "lowest kept neighbour, the base drops row 2": (1, 5, [(0, 2)], [(0, 1), (1, 4), (2, 4), (3, 4)]),
    "one row, kept": (1, 1, [], []),
    "one row, dropped": (1, 1, [(0, 0)], []),
    "path of 40, every fourth row has a base partner": (10, 40, [(i, 4 * i) for i in range(10)], [(i, i + 1) for i in range(39)]),
}


@pytest.mark.parametrize("shape", list(ADMIT))
def test_admission(gpu, mse, orc, shape):
    nb, m, cross_edges, among_edges = ADMIT[shape]
    d = 64
    x = gram_rows(nb + m, [(b, nb + j) for b, j in cross_edges] + [(nb + a, nb + c) for a, c in among_edges], d)
    w = World(mse, orc, x[:nb], x[nb:], d)
    thr = mse.scale_dot_result(0.9)
    cw = w.want(thr)
    aw = self_ref.pairs_from_scores(self_ref.score_matrix(orc, w.inc), thr)
    assert sorted(zip(cw[0].tolist(), cw[1].tolist())) == sorted(cross_edges), "the bases must realise the wanted cross pairs"
    assert sorted(zip(aw[0].tolist(), aw[1].tolist())) == sorted(among_edges), "the batch must realise the wanted pair graph"
    qs = mse.Searcher(w.q)
    for with_among in (True, False):
        al, ah = (aw[0], aw[1]) if with_among else (None, None)
        kept, rb, ri = ref.admit(m, cw[1], cw[0], al, ah)
        rounds, kept_by_rounds = ref.admit_rounds(m, cw[1], al, ah)
        assert np.array_equal(kept, kept_by_rounds)
        out = []
        for run in range(2):
            cross = w.join(thr, mode=mse.MODE_MFMA if run else mse.MODE_AUTO)
            same_pairs(cross, cw, shape)
            among = qs.near_duplicates(thr) if with_among else None
            adm = cross.admit(among)
            assert adm.rep_base.dtype == np.uint32 and adm.rep_incoming.dtype == np.uint32
            assert len(adm.kept) == m and np.array_equal(adm.kept.to_mask(), kept), (shape, with_among)
            assert np.array_equal(adm.rep_base, rb) and np.array_equal(adm.rep_incoming, ri), (shape, with_among)
            assert w.s.join_stats()["rounds"] == rounds, (shape, with_among, w.s.join_stats(), rounds)
            dropped = int((adm.rep_incoming != np.arange(m)).sum())
            assert adm.kept.count + dropped == m
            again = cross.admit(among)                    # the list is immutable: the same answer
            out.append((adm.kept.to_mask().tobytes(), adm.rep_base.tobytes(), adm.rep_incoming.tobytes()))
            assert out[-1] == (again.kept.to_mask().tobytes(), again.rep_base.tobytes(), again.rep_incoming.tobytes())
            for h in (again, adm, among, cross):
                if h is not None:
                    h.close()
        assert out[0] == out[1], "two runs give the same bytes"
    if shape.startswith("chain"):
        assert ref.admit(m, cw[1], cw[0], aw[0], aw[1])[0].tolist() == [False, True]
    if shape.startswith("path of 40"):
        k = ref.admit(m, cw[1], cw[0], aw[0], aw[1])[0]
        assert k.tolist() == [i % 4 in (1, 3) for i in range(40)] and ref.admit_rounds(m, cw[1], aw[0], aw[1])[0] == 3
    qs.close()
    w.close()


# ---- 7. select ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 255, 257])
def test_select(gpu, mse, orc, m):
    d = 64
    rows = bits(orc, unit_rows(m, d, 60 + m))
    vl = mse.VectorList.from_f16s(rows, d)
    rng = np.random.default_rng(m)
    cases = [("none", np.zeros(m, bool)), ("all", np.ones(m, bool)), ("some", rng.random(m) < 0.5)]
    if m > 1:
        cases.append(("short", np.ones(m // 2, bool)))          # a filter shorter than the list excludes the later rows
    for name, mask in cases:
        f = mse.RowFilter(mask)
        got = vl.select(f)
        full = np.zeros(m, bool)
        full[:mask.size] = mask
        assert len(got) == int(full.sum()) and got.d_emb == d, name
        assert np.array_equal(got.rows(0, len(got)), rows[full]), name
        got.close()
        f.close()
    vl.close()


# ---- 8. insert only what is new ----------------------------------------------------------------------------------------------------

def test_insert_unique_rows(gpu, mse, orc):
    n, d, m = 3000, 1152, 200
    x = clustered_rows(orc, n, d, n_centres=50, noise=0.5, seed=17).astype(np.float64)
    rows = orc.f16_bits(x.astype(np.float32))
    rng = np.random.default_rng(5)
    cents, T, dpc, _ = make_pq(orc, d)
    cfg = mse.IndexBuildConfig(r=32, l=64, maxc=250)
    vl0 = mse.VectorList.from_f16s(rows, d)
    s0 = mse.Searcher(vl0)
    g0 = mse.BuildGraph(n, 32)
    g0.random_fill(9)
    med = mse.medioid(vl0)
    g0.build(s0, np.random.default_rng(9).permutation(n).astype(np.uint32), med, cfg, 1024)
    h0 = g0.to_host()
    g0.close()
    gpq = mse.ProductQuantizer(cents, T, dpc, d)
    codes = gpq.quantize_batch(orc.f16_to_f32(rows))
    desc = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    url = np.ones(n, np.uint8)
    slots = rng.choice(np.setdiff1d(np.arange(n), [med]), m, replace=False).astype(np.uint32)
    dead = np.zeros(n, bool)
    dead[slots] = True
    # the batch: 40 rows copy live resident rows, 20 copy earlier rows of the batch, the rest is new (far from the index: other centres)
    xq = unit_rows(m, d, 77)
    live_ids = np.flatnonzero(~dead)
    from_base = rng.choice(m, 40, replace=False)
    srcs = rng.choice(live_ids, 40, replace=False)
    plant_cross(x, xq, list(zip(srcs.tolist(), from_base.tolist())), noise=0.1)
    rest = np.setdiff1d(np.arange(20, m), from_base)
    later = rng.choice(rest, 20, replace=False)
    plant(xq, [(int(rng.integers(0, j)), int(j)) for j in later], seed=6, noise=0.1)
    inc = orc.f16_bits(xq.astype(np.float32))
    new_desc = rng.integers(0, 256, size=(m, 4), dtype=np.uint8)
    new_url = (rng.random(m) > 0.3).astype(np.uint8)
    thr = mse.scale_dot_result(0.9)
    # the walk
    cw = ref.cross_pairs(orc, rows, inc, thr, ~dead)
    aw = self_ref.pairs_from_scores(self_ref.score_matrix(orc, inc), thr)
    kept, rb, ri = ref.admit(m, cw[1], cw[0], aw[0], aw[1])
    assert 40 <= int((~kept).sum()) <= 60 and (rb[from_base] != NONE).all() and not kept[from_base].any()
    assert (~kept[later]).sum() >= 1 and (rb != NONE).sum() >= 40
    k = int(kept.sum())

    def index():
        vl = mse.VectorList.from_f16s(rows, d)
        s = mse.Searcher(vl)
        gc = mse.Codes(codes, desc)
        g = mse.DeviceGraph(mse.IndexGraph(h0.adj, h0.deg), url)
        assert g.delete_rows(s, slots, cfg)["deleted"] == m
        return vl, s, gc, g

    vl1, s1, gc1, g1 = index()
    out = g1.insert_unique_rows(s1, slots, inc, thr, cfg, med, quantizer=gpq, codes=gc1, descriptors=new_desc, has_url=new_url, batch=64)
    assert np.array_equal(out["kept"], kept) and np.array_equal(out["rep_base"], rb) and np.array_equal(out["rep_incoming"], ri)
    assert np.array_equal(out["unused_slots"], slots[k:]) and out["inserted"] == k
    vl2, s2, gc2, g2 = index()
    st = g2.insert_rows(s2, slots[:k], inc[kept], cfg, med, quantizer=gpq, codes=gc2, descriptors=new_desc[kept], has_url=new_url[kept], batch=64)
    assert st == {"inserted": out["inserted"], "batches": out["batches"]}
    ha, hb = g1.to_host(), g2.to_host()
    assert np.array_equal(ha.adj, hb.adj) and np.array_equal(ha.deg, hb.deg)
    assert np.array_equal(vl1.rows(0, n), vl2.rows(0, n)) and np.array_equal(vl1.rows(0, n)[slots[:k]], inc[kept])
    ca, cb = gc1.read_rows(0, n, descriptors=True), gc2.read_rows(0, n, descriptors=True)
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and np.array_equal(ca[1][slots[:k]], new_desc[kept])
    assert np.array_equal(g1.deleted(), g2.deleted()) and int(g1.deleted().sum()) == m - k
    # the same batch again: every row now has a partner in the index
    again = g1.near_duplicates_of(s1, inc, thr)
    adm = again.admit()
    assert adm.kept.count == 0 and (adm.rep_base != NONE).all()
    out2 = g1.insert_unique_rows(s1, slots[k:], inc[:m - k], thr, cfg, med, quantizer=gpq, codes=gc1, descriptors=new_desc[:m - k],
                                 has_url=new_url[:m - k])
    assert out2["inserted"] == 0 and not out2["kept"].any() and np.array_equal(out2["unused_slots"], slots[k:])
    adm.close()
    again.close()
    for g in (g1, g2):
        g.close()


# ---- 9. errors and overflow --------------------------------------------------------------------------------------------------------

def test_errors_and_overflow(gpu, mse, orc):
    from mse import ffi
    n, m, d = TILE + 9, TILE + 3, 64
    xb, xq = unit_rows(n, d, 5), unit_rows(m, d, 6)
    plant_cross(xb, xq, [(1, 2), (3, 130), (130, 4)], noise=0.05)
    w = World(mse, orc, xb, xq, d)
    thr = mse.scale_dot_result(0.9)
    want = w.want(thr)
    assert want[0].size >= 3
    for mode in MODES:
        with pytest.raises(mse.MseError, match="max_pairs"):
            w.join(thr, mode=getattr(mse, mode), max_pairs=want[0].size - 1)
        assert w.s.join_stats()["kept"] == want[0].size            # the true count, so the caller can ask again
        p = w.join(thr, mode=getattr(mse, mode), max_pairs=want[0].size)   # the searcher answers as a fresh one
        same_pairs(p, want, mode)
        p.close()
    L = ffi.lib()
    with pytest.raises(mse.MseError, match="null searcher"):
        ffi.check_ptr(L.mse_join_cross(None, w.q._h, thr, None, mse.MODE_AUTO, 1 << 32))
    with pytest.raises(mse.MseError, match="null incoming base"):
        ffi.check_ptr(L.mse_join_cross(w.s._h, None, thr, None, mse.MODE_AUTO, 1 << 32))
    wide = mse.VectorList.from_f16s(np.zeros((3, 128), np.uint16), 128)
    long = mse.RowFilter(np.ones(n + 1, bool))
    with pytest.raises(mse.MseError, match="128 wide, the base's 64"):
        w.s.near_duplicates_of(wide, thr, within=long, mode=7)      # the width comes before the filter and the mode
    with pytest.raises(mse.MseError, match="filter is longer than the base"):
        w.join(thr, within=long, mode=7)                            # the filter before the mode
    with pytest.raises(mse.MseError, match="unknown mode"):
        w.join(thr, mode=7)
    with pytest.raises(TypeError):
        w.join(thr, within=np.ones(n, bool))
    if gpu >= 2:
        ffi.check(L.mse_set_device(1))
        other_q = mse.VectorList.from_f16s(w.inc, d)
        other_f = mse.RowFilter(np.ones(n, bool))
        ffi.check(L.mse_set_device(0))
        with pytest.raises(mse.MseError, match="another device"):
            w.s.near_duplicates_of(other_q, thr)
        with pytest.raises(mse.MseError, match="another device"):
            w.join(thr, within=other_f)
        other_q.close()
        other_f.close()
    # the self-list calls on a cross list name the call that applies
    cross = w.join(thr)
    same_pairs(cross, want, "after the errors")
    for call in (cross.duplicates, cross.groups, cross.representatives):
        with pytest.raises(mse.MseError, match="mse_pairs_admit"):
            call()
    # admission: the kinds, the row counts, the output
    qs = mse.Searcher(w.q)
    among = qs.near_duplicates(thr)
    mine = w.s.near_duplicates(thr)                                  # a self list over n rows, not m
    with pytest.raises(mse.MseError, match="must be a cross list"):
        among.admit()
    with pytest.raises(mse.MseError, match="must be a self list"):
        cross.admit(cross)
    with pytest.raises(mse.MseError, match=f"over {n} rows, the cross list over {m} incoming rows"):
        cross.admit(mine)
    with pytest.raises(mse.MseError, match="null kept_out"):
        ffi.check(L.mse_pairs_admit(cross._h, among._h, None, None, None))
    with pytest.raises(TypeError):
        cross.admit(np.zeros(3))
    adm = cross.admit(among)
    kept, rb, ri = ref.admit(m, want[1], want[0], *among.read()[:2])
    assert np.array_equal(adm.kept.to_mask(), kept) and np.array_equal(adm.rep_base, rb) and np.array_equal(adm.rep_incoming, ri)
    # select: a filter longer than the base
    with pytest.raises(mse.MseError, match="filter is longer than the base"):
        w.q.select(long)
    with pytest.raises(TypeError):
        w.q.select(np.ones(m, bool))
    for h in (adm, mine, among, qs, cross, long, wide):
        h.close()
    # an empty side: an empty list over the incoming rows, and admission keeps every row
    empty = mse.VectorList.from_f16s(np.zeros((0, d), np.uint16), d)
    s0 = mse.Searcher(empty)
    for s, q, rows, base_rows in ((w.s, empty, 0, n), (s0, w.q, m, 0), (s0, empty, 0, 0)):
        for mode in MODES:
            p = s.near_duplicates_of(q, thr, mode=getattr(mse, mode))
            assert len(p) == rows and p.count == 0 and p.kind == 1 and p.base_rows == base_rows and p.read()[0].size == 0
            adm = p.admit()
            assert len(adm.kept) == rows and adm.kept.count == rows and (adm.rep_base == NONE).all()
            assert np.array_equal(adm.rep_incoming, np.arange(rows, dtype=np.uint32))
            adm.close()
            p.close()
    s0.close()
    empty.close()
    w.close()
