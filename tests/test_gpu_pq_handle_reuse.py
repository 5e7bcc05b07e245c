"""One ProductQuantizer for a server's lifetime (the method of tests/test_gpu_handle_reuse.py: poison, then probe).

The quantiser's flat scan lives on buffers that are reused between calls and not cleared -- the uploaded queries and scales, transformed
queries and tables, the lazily made scratch searcher, the lane searchers that are bound to the base of the call that made them, the
certificate flags -- and on one sticky switch (eight queries per pass -> four).  One quantiser goes through code sets of 12345, 4097, 70
and 1 vectors, with and without descriptors and scales, with and without a re-scoring Searcher, filtered and unfiltered, in batches of
every shape; POISON queries are the pool's queries x 1000, PROBE queries the same x 0.001, so that whatever a poison call leaves behind
would win a probe call.  Every answer equals the oracle pipeline the other PQ tests use and the same call on a fresh quantiser,
`last_uncertified` included."""
import numpy as np
import pytest

from conftest import SEED_BASE, make_pq

pytestmark = pytest.mark.gpu
D = 1152
I64_MIN = np.iinfo(np.int64).min
ID_NONE = 0xFFFFFFFF
SCALES = np.array([0.5, 0, -0.25, 0.125], np.float32) / np.float32(512)


class Flat:
    """codec, code sets, bases, query pools and the oracle's numbers (tables, ADC scores) behind every expectation"""

    SETS = {"big": (12345, True), "mid": (4097, False), "small": (70, True), "one": (1, False)}

    def __init__(self, orc, mse):
        self.orc, self.mse = orc, mse
        rng = np.random.default_rng(20262)
        self.codec = make_pq(orc)
        self.opq = orc.PQ(*self.codec)
        self.codes = {name: rng.integers(0, 256, size=(n, 64), dtype=np.uint8) for name, (n, _) in self.SETS.items()}
        self.desc = {name: rng.integers(0, 256, size=(n, 4), dtype=np.uint8) if has else None for name, (n, has) in self.SETS.items()}
        self.base = {"big": orc.gen_rows_f16(SEED_BASE, 0, 12345), "mid": orc.gen_rows_f16(SEED_BASE, 50000, 4097)}
        unit = (rng.standard_normal((9, D)) / np.sqrt(D)).astype(np.float32)
        self.pools = {"poison": unit * np.float32(1000), "probe": unit * np.float32(1e-3)}
        self.masks = {"dense": rng.random(12345) < 0.7, "few": np.zeros(12345, bool)}
        self.masks["few"][rng.choice(12345, 23, replace=False)] = True
        self._lut, self._adc = {}, {}
        # 4097 vectors end in a group of ONE, whose maximum is that vector's score: it gets the code row, out of 20000 random ones, whose
        # worst score over the poison queries is best -- so that this group's slot, too, is left holding a value a probe call cannot reach
        cand = rng.integers(0, 256, size=(20000, 64), dtype=np.uint8)
        worst = np.min([self.opq.asymmetric_dot_product(self.lut("poison", j), cand) for j in range(9)], axis=0)
        self.codes["mid"][-1] = cand[int(np.argmax(worst))]
        self.dev = None
        self._checked = False

    def lut(self, pool, j):
        if (pool, j) not in self._lut:
            self._lut[(pool, j)] = self.opq.preprocess_query(self.pools[pool][j])
        return self._lut[(pool, j)]

    def adc(self, pool, j, cset, scaled):
        """the oracle's ADC score of every vector of a code set (+ descriptor bias when the call passes scales and the set has descriptors)"""
        key = (pool, j, cset, scaled)
        if key not in self._adc:
            codes, desc = self.codes[cset], self.desc[cset]
            self._adc[key] = (self.opq.adc_desc(self.lut(pool, j), codes, desc, SCALES) if scaled and desc is not None
                              else self.opq.asymmetric_dot_product(self.lut(pool, j), codes))
        return self._adc[key]

    def check_poison(self):
        """the smallest group maximum (64 vectors) any poison query leaves in the scan's scratch, and the smallest score a poison call
        returns after the exact re-score, are above the largest score of any vector under any probe query -- ADC or re-scored, with
        the largest descriptor bias added"""
        if self._checked:
            return
        gmin = None
        for cset in ("big", "mid"):
            for scaled in (True, False):
                for j in range(9):
                    a = self.adc("poison", j, cset, scaled)
                    n = len(a)
                    pad = np.full((n + 63) // 64 * 64, I64_MIN, np.int64)
                    pad[:n] = a
                    g = int(pad.reshape(-1, 64).max(axis=1).min())
                    gmin = g if gmin is None else min(gmin, g)
        pmax = max(int(self.adc("probe", j, cset, True).max()) for cset in self.SETS for j in range(9))
        bias = int(np.abs(SCALES).sum() * 255 * 2.0 ** 32) + 4
        for name, base in self.base.items():
            for j in range(4):
                pmax = max(pmax, int(self.orc.score_all(base, self.orc.f16_bits(self.pools["probe"][j])).max()) + bias)
        rmin = min(int(self.want("big", "poison", range(4), 200, 64, True, True)[0].min()),
                   int(self.want("mid", "poison", range(4), 200, 64, True, True)[0].min()))
        print("smallest poison group maximum %.3g, smallest re-scored poison answer %.3g, largest probe score %.3g (units of 2^32)"
              % (gmin / 2.0 ** 32, rmin / 2.0 ** 32, pmax / 2.0 ** 32))
        assert gmin > pmax and rmin > pmax
        self._checked = True

    def want(self, cset, pool, js, r, k, scaled, rescored, allow=None):
        """the oracle pipeline: ADC (+ bias) over the (allowed) vectors -> top-r -> with a searcher: exact fast_dot of the f16 query
        (+ bias) over those r, ordered (score desc, id asc) -> top-k, padded (INT64_MIN, ID_NONE)"""
        orc = self.orc
        r = max(r, k)
        desc = self.desc[cset]
        use_bias = scaled and desc is not None
        ws = np.full((len(js), k), I64_MIN, np.int64)
        wi = np.full((len(js), k), ID_NONE, np.uint32)
        allowed = None if allow is None else np.flatnonzero(self.masks[allow])
        for o, j in enumerate(js):
            approx = self.adc(pool, j, cset, scaled)
            if allowed is not None:
                s, i = orc.topk_from_scores(approx[allowed], min(r, len(allowed)))
                i = allowed[i].astype(np.uint32)
            else:
                s, i = orc.topk_from_scores(approx, min(r, len(approx)))
            if rescored:
                exact = orc.score_rows(self.base[cset], i, orc.f16_bits(self.pools[pool][j]))
                if use_bias:
                    exact = exact + np.array([orc.descriptor_product(SCALES, desc, int(c)) for c in i], np.int64)
                order = np.lexsort((i, -exact))
                s, i = exact[order], i[order]
            m = min(k, len(i))
            ws[o, :m], wi[o, :m] = s[:m], i[:m]
        return ws, wi

    def device(self):
        if self.dev is None:
            mse = self.mse
            self.dev = {"codes": {n: mse.Codes(self.codes[n], self.desc[n]) for n in self.SETS},
                        "vl": {n: mse.VectorList.from_f16s(b, D) for n, b in self.base.items()},
                        "filters": {n: mse.RowFilter(m) for n, m in self.masks.items()}}
        return self.dev


@pytest.fixture(scope="module")
def flat(orc, mse):
    return Flat(orc, mse)


def step(cset, pool, js, r, k, scaled=False, searcher=None, allow=None, uncertified=None):
    """one scan_topk_batch(_filtered) call: queries js of a pool over a code set; searcher: None (the quantiser's own scratch and
    lanes) or the name of the base whose long-lived Searcher re-scores; uncertified: what last_uncertified must say (None: the fresh
    quantiser's)"""
    return dict(cset=cset, pool=pool, js=tuple(js), r=r, k=k, scaled=scaled, searcher=searcher, allow=allow, uncertified=uncertified)


def call(flat, gpq, searchers, st):
    dev = flat.device()
    qs = np.ascontiguousarray(flat.pools[st["pool"]][list(st["js"])])
    s = searchers[st["searcher"]] if st["searcher"] else None
    sc = SCALES if st["scaled"] else None
    codes = dev["codes"][st["cset"]]
    if st["allow"]:
        got = gpq.scan_topk_batch_filtered(codes, dev["filters"][st["allow"]], qs, st["r"], st["k"], s, sc)
    else:
        got = gpq.scan_topk_batch(codes, qs, st["r"], st["k"], s, sc)
    return got[0], got[1], gpq.last_uncertified


def run_sequence(flat, seq, compare_uncertified=True):
    mse = flat.mse
    flat.check_poison()
    dev = flat.device()
    gpq = mse.ProductQuantizer(*flat.codec)
    searchers = {n: mse.Searcher(vl) for n, vl in dev["vl"].items()}
    for n, st in enumerate(seq):
        where = (n,) + tuple(st.values())
        ws, wi = flat.want(st["cset"], st["pool"], st["js"], st["r"], st["k"], st["scaled"], st["searcher"] is not None, st["allow"])
        sc, ids, unc = call(flat, gpq, searchers, st)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), ("long-lived quantiser differs from the oracle", where)
        fpq = mse.ProductQuantizer(*flat.codec)
        fs = {st["searcher"]: mse.Searcher(dev["vl"][st["searcher"]])} if st["searcher"] else {}
        fsc, fids, func = call(flat, fpq, fs, st)
        fpq.close()
        for s in fs.values():
            s.close()
        assert np.array_equal(fids, wi) and np.array_equal(fsc, ws), ("fresh quantiser differs from the oracle", where)
        if compare_uncertified:
            assert unc == func, (where, unc, func)
        if st["uncertified"] is not None:
            assert unc == st["uncertified"], (where, unc)
    gpq.close()
    for s in searchers.values():
        s.close()


P, Q = "poison", "probe"


def test_code_sets_of_other_sizes_and_no_scales_after_scales(gpu, flat):
    """9 poison queries (eight per pass + 1) with scales over 12345 vectors, r = 200, k = 64 -> 3 probes over 70 vectors (fewer groups
    than r) -> 1 probe over one vector at k = 2 -> 4 probes over 4097 vectors WITHOUT scales, which the previous batch's must not reach"""
    poison = step("big", P, range(9), 200, 64, scaled=True)
    run_sequence(flat, [poison, step("small", Q, range(3), 200, 64, scaled=True),
                        poison, step("one", Q, [0], 3, 2),
                        poison, step("mid", Q, range(4), 200, 64),
                        poison, step("big", Q, range(4), 200, 64),                 # the same codes (with descriptors), no scales
                        step("small", Q, range(3), 200, 10), step("big", Q, range(9), 200, 64, scaled=True)])


def test_scratch_lanes_and_searchers_in_turn(gpu, flat):
    """searcher=None (the quantiser's own scratch and lanes) -> a Searcher over the 12345-row base (re-scored; the lanes are re-made on
    that base) -> a Searcher over the 4097-row base with the 4097 codes (the lanes point at another base) -> None again"""
    run_sequence(flat, [step("big", P, range(9), 200, 64, scaled=True),
                        step("big", Q, range(9), 200, 64, scaled=True, searcher="big"),
                        step("big", P, range(4), 200, 64, scaled=True, searcher="big"),
                        step("mid", Q, range(4), 200, 64, scaled=True, searcher="mid"),       # (no descriptors: the scales add nothing)
                        step("mid", P, range(4), 200, 64, searcher="mid"),
                        step("mid", Q, range(9), 120, 10),
                        step("big", Q, range(5), 120, 10, searcher="big"),
                        step("big", Q, range(4), 120, 10, scaled=True),
                        step("mid", Q, range(1), 120, 10, searcher="mid"),
                        step("big", Q, range(2), 120, 10, scaled=True, searcher="big")])


def test_batch_sizes_in_turn(gpu, flat):
    """9 -> 4 -> 3 -> 2 -> 1 -> 8 queries over one code set: eights, fours, a pair, a single one, and the certificate flags of the batch before"""
    seq = [step("big", P, range(9), 120, 10, scaled=True)]
    for m in (4, 3, 2, 1, 8):
        seq.append(step("big", Q, range(m), 120, 10, scaled=True))
    seq += [step("big", P, range(8), 120, 10), step("big", Q, range(1, 4), 10, 10), step("big", Q, range(8), 10, 10, scaled=True)]
    run_sequence(flat, seq)


def test_filtered_between_unfiltered(gpu, flat):
    """an unfiltered poison batch -> a dense filter -> a filter with fewer allowed vectors than k (the rest is padding, not the poison
    batch's ids) -> an unfiltered probe; with and without a re-scoring Searcher"""
    assert flat.masks["few"].sum() == 23
    run_sequence(flat, [step("big", P, range(9), 200, 64, scaled=True),
                        step("big", Q, range(5), 200, 64, scaled=True, allow="dense"),
                        step("big", Q, range(5), 200, 64, scaled=True, allow="few"),
                        step("big", Q, range(9), 200, 64, scaled=True),
                        step("big", P, range(8), 200, 64, scaled=True, searcher="big"),
                        step("big", Q, range(4), 200, 64, scaled=True, searcher="big", allow="dense"),
                        step("big", Q, range(4), 200, 64, scaled=True, searcher="big", allow="few"),
                        step("big", Q, range(1), 200, 64, allow="few"),
                        step("big", Q, range(3), 200, 64, scaled=True, searcher="big")])
    ws, wi = flat.want("big", Q, range(5), 200, 64, True, False, "few")
    assert np.all(wi[:, 23:] == ID_NONE) and np.all(ws[:, 23:] == I64_MIN) and np.all(flat.masks["few"][wi[:, :23]])


def test_tied_codes_switch_to_four_per_pass_and_answers_stay(gpu, flat, mse, orc):
    """Seven distinct code rows: thousands of vectors share the r-th score exactly, so no certificate can hold (strict >) as soon as one
    group is excluded.  Eight per pass at r = k = 10 nominate 2 r + 112 = 132 groups and read the key of one more, so 133 groups -- 8512
    vectors -- is the smallest set with an excluded group: all eight queries are repeated through the exact scan, and the handle stays
    with four per pass from then on.  The spread-out batches of eight before and after it return the oracle's answers either way."""
    flat.check_poison()
    rng = np.random.default_rng(91)
    n, r, k = 133 * 64, 10, 10
    tied = rng.integers(0, 256, size=(7, 64), dtype=np.uint8)[rng.integers(0, 7, size=n)]
    gt = mse.Codes(tied, None)
    dev = flat.device()
    gpq = mse.ProductQuantizer(*flat.codec)

    def spread(pool, r_):
        ws, wi = flat.want("big", pool, range(8), r_, k, True, False)
        sc, ids = gpq.scan_topk_batch(dev["codes"]["big"], flat.pools[pool][:8], r_, k, None, SCALES)
        assert np.array_equal(ids, wi) and np.array_equal(sc, ws), (pool, r_)
        return gpq.last_uncertified

    def on_tied(pool, m):
        sc, ids = gpq.scan_topk_batch(gt, flat.pools[pool][:m], r, k)
        for j in range(m):
            ws, wi = orc.topk_from_scores(flat.opq.asymmetric_dot_product(flat.lut(pool, j), tied), k)
            assert np.array_equal(ids[j], wi) and np.array_equal(sc[j], ws), (pool, m, j)
        return gpq.last_uncertified

    assert spread(P, 200) == 0                                   # eight per pass, every group nominated: certified
    assert on_tied(P, 8) == 8                                    # all eight repeated: the switch is set
    assert spread(Q, 200) == 0                                   # four + four now: the oracle's answers
    assert spread(Q, 10) == spread(Q, 10)                        # ... and a real certificate (74 of 193 groups), twice the same
    assert on_tied(Q, 8) == 8                                    # 4 + 4 on the tied codes: 75 < 133 groups, none certified
    assert on_tied(Q, 3) == 0                                    # a pair and a single one: exact scans, nothing to certify
    assert spread(P, 200) == 0
    gpq.close()
    gt.close()
