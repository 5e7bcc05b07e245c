"""Insert rows into freed slots of a live graph index (mse_graph_insert_rows, include/mse.h): the linked graph edge for edge against the
CPU oracle's build continued on the restated delete; rows, codes, descriptors and flags through every request-path entry point against
a fresh upload of the new arrays and against the oracle; the raised norm bound; capacity from spare slots; errors that leave everything
untouched; and an insert racing requests in flight."""
import threading
import types

import numpy as np
import pytest

from test_gpu_filtered_graph import Index, SCALES, sorted_cut, clustered_rows
from test_gpu_graph_delete import request_calls, same_answers, cfgs
from test_graph_delete_host import restate_delete, same_graph, property_set, oracle_graph

pytestmark = pytest.mark.gpu
D, N, M, K = 1152, 6000, 500, 10
NONE = 0xFFFFFFFF
KW = dict(r=32, l=64, maxc=250)
IKW = dict(r=16, l=64, maxc=250)                                # the Index fixture's graph has stride 16


# ---- 1. graph parity with the oracle ------------------------------------------------------------------------------------------------
class World:
    """6 000 clustered rows, the graph built on the device as test_slot_reuse builds it, 500 rows (not the medioid) deleted by the
    restated rule on the CPU, 500 fresh vectors, and the oracle's build continued over the slots -- computed once per batch size."""

    def __init__(self, mse, orc):
        self.rows = orc.f16_bits(clustered_rows(orc, N, D, n_centres=40, noise=0.5, seed=31))
        vl = mse.VectorList.from_f16s(self.rows, D)
        s = mse.Searcher(vl)
        self.ocfg, self.mcfg = cfgs(orc, mse, **KW)
        g = mse.BuildGraph(N, 32)
        g.random_fill(32)
        self.med = mse.medioid(vl)
        g.build(s, np.random.default_rng(32).permutation(N).astype(np.uint32), self.med, self.mcfg, 512)
        h = g.to_host()
        g.close()
        self.adj, self.deg = h.adj, h.deg
        rng = np.random.default_rng(33)
        self.slots = rng.choice(np.setdiff1d(np.arange(N), [self.med]), M, replace=False).astype(np.uint32)
        self.dead = np.zeros(N, bool)
        self.dead[self.slots] = True
        self.wa, self.wd, _ = restate_delete(orc, self.rows, self.adj, self.deg, self.dead, self.ocfg)
        self.fresh = orc.f16_bits(clustered_rows(orc, M, D, n_centres=40, noise=0.5, seed=34))
        self.rows2 = self.rows.copy()
        self.rows2[self.slots] = self.fresh
        self.orc, self._want = orc, {}

    def want(self, batch):
        if batch not in self._want:
            a, d = self.wa.copy(), self.wd.copy()
            self.orc.build_graph(self.rows2, a, d, self.slots, self.med, self.ocfg, batch)
            self._want[batch] = (a, d)
        return self._want[batch]

    def deleted_graph(self, mse, searcher):
        g = mse.BuildGraph(N, 32, mse.IndexGraph(self.adj, self.deg))
        assert g.delete_rows(searcher, self.slots, self.mcfg)["deleted"] == M
        return g


@pytest.fixture(scope="module")
def world(gpu, mse, orc):
    return World(mse, orc)


def check_inserted(w, g, vl, batch, st):
    h = g.to_host()
    wa, wd = w.want(batch)
    assert same_graph(h.adj, h.deg, wa, wd), f"batch {batch}: the device graph differs from the oracle's continued build"
    assert not g.deleted().any() and (h.deg[w.slots] > 0).all()
    assert np.array_equal(vl.rows(0, N), w.rows2)               # the new rows in their slots, every other row as it was
    assert st == {"inserted": M, "batches": -(-M // batch)}
    return h


@pytest.mark.parametrize("batch", [1, 64])
def test_insert_matches_the_oracle(world, mse, orc, batch):
    """owned base (from_f16s), host rows: delete 500, insert 500 fresh vectors == restate_delete, then orc.build_graph over the slots"""
    w = world
    vl = mse.VectorList.from_f16s(w.rows, D)
    s = mse.Searcher(vl)
    g = w.deleted_graph(mse, s)
    h1 = g.to_host()
    assert same_graph(h1.adj, h1.deg, w.wa, w.wd)
    st = g.insert_rows(s, w.slots, w.fresh, w.mcfg, w.med, batch=batch)
    check_inserted(w, g, vl, batch, st)
    if batch == 64:                                             # the batch decides, as it does in the build
        assert not same_graph(*w.want(1), *w.want(64))
    g.close()


def test_insert_wrapped_base_and_device_rows(world, mse, orc):
    """the base as a wrapped device tensor, and the rows as a device tensor: the same graph as the host-pointer call, array for array"""
    import torch
    w = world
    vl = mse.VectorList.from_f16s(w.rows, D)
    s = mse.Searcher(vl)
    g = w.deleted_graph(mse, s)
    st = g.insert_rows(s, w.slots, w.fresh, w.mcfg, w.med, batch=64)
    ref = check_inserted(w, g, vl, 64, st)
    g.close()
    # wrapped base, host rows
    t = torch.from_numpy(w.rows.view(np.int16).copy()).cuda()
    wl = mse.VectorList.wrap_device(t.data_ptr(), N, D, keepalive=t)
    ws = mse.Searcher(wl)
    g = w.deleted_graph(mse, ws)
    st = g.insert_rows(ws, w.slots, w.fresh, w.mcfg, w.med, batch=64)
    h = check_inserted(w, g, wl, 64, st)
    assert np.array_equal(h.adj, ref.adj) and np.array_equal(h.deg, ref.deg)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint16), w.rows2)   # the caller's tensor holds the new rows
    g.close()
    # owned base, rows resident on the device (f16 tensor, as an encoder leaves them)
    vl2 = mse.VectorList.from_f16s(w.rows, D)
    s2 = mse.Searcher(vl2)
    g = w.deleted_graph(mse, s2)
    dev_rows = torch.from_numpy(w.fresh.view(np.float16).copy()).cuda()
    st = g.insert_rows(s2, w.slots, dev_rows, w.mcfg, w.med, batch=64)
    h = check_inserted(w, g, vl2, 64, st)
    assert np.array_equal(h.adj, ref.adj) and np.array_equal(h.deg, ref.deg)
    g.close()


# ---- 2. codes, descriptors, flags: the request path --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def index(gpu, mse, orc):
    return Index(mse, orc, D, 31)


class Live:
    """A private, mutable copy of the Index fixture's device objects (the fixture itself is shared and stays as it was): base,
    codes + descriptors, graph with has_url; 500 slots deleted on the device."""

    def __init__(self, mse, orc, ix, seed, with_desc=True):
        rng = np.random.default_rng(seed)
        self.ix = ix
        self.vecs = mse.VectorList.from_f16s(ix.base, D)
        self.searcher = mse.Searcher(self.vecs)
        self.gcodes = mse.Codes(ix.codes, ix.desc if with_desc else None)
        self.g = mse.DeviceGraph(mse.IndexGraph(ix.adj, ix.degs), ix.has_url)
        self.slots = rng.choice(np.setdiff1d(np.arange(ix.n), ix.starts), M, replace=False).astype(np.uint32)
        self.dead = np.zeros(ix.n, bool)
        self.dead[self.slots] = True
        self.ocfg, self.mcfg = cfgs(orc, mse, **IKW)
        assert self.g.delete_rows(self.searcher, self.slots, self.mcfg)["deleted"] == M
        self.fresh = orc.f16_bits(clustered_rows(orc, M, D, n_centres=48, seed=seed + 1))
        self.new_desc = rng.integers(0, 256, size=(M, 4), dtype=np.uint8)
        self.new_url = (rng.random(M) > 0.3).astype(np.uint8)
        self.new_url[:12:2], self.new_url[1:12:2] = 1, 0        # the rows the queries are copies of: six with a url, six without
        self.url_deleted = (ix.has_url.astype(bool) & ~self.dead).astype(np.uint8)
        self.start = int(ix.starts[0])

    def view(self, **kw):
        """what request_calls reads from an index, with this copy's objects (and whatever kw replaces)"""
        ix = self.ix
        d = dict(searcher=self.searcher, gpq=ix.gpq, gcodes=self.gcodes, qh=ix.qh, qs=ix.qs, starts=ix.starts, luts=ix.luts)
        d.update(kw)
        return types.SimpleNamespace(**d)

    def twin(self, mse, rows, codes, desc, adj, deg, url):
        vl = mse.VectorList.from_f16s(rows, D)
        return types.SimpleNamespace(vecs=vl, searcher=mse.Searcher(vl), gcodes=mse.Codes(codes, desc), g=mse.DeviceGraph(mse.IndexGraph(adj, deg), url))

    def close(self):
        self.g.close()


def test_search_after_insert(index, mse, orc):
    """rows, codes, descriptors and has_url of the inserted index == a fresh upload of the new arrays, through every request-path entry
    point bit for bit, and == the oracle on those arrays.  The queries are copies of twelve inserted rows: the six with has_url = 1
    must be found, none of the inserted rows with has_url = 0 may appear."""
    ix = index
    lv = Live(mse, orc, ix, 71)
    st = lv.g.insert_rows(lv.searcher, lv.slots, lv.fresh, lv.mcfg, lv.start, quantizer=ix.gpq, codes=lv.gcodes, descriptors=lv.new_desc,
                          has_url=lv.new_url, batch=64)
    assert st["inserted"] == M
    h = lv.g.to_host()
    rows2, codes2, desc2, url2 = ix.base.copy(), ix.codes.copy(), ix.desc.copy(), lv.url_deleted.copy()
    rows2[lv.slots], desc2[lv.slots], url2[lv.slots] = lv.fresh, lv.new_desc, lv.new_url
    new_codes = ix.gpq.quantize_batch(orc.f16_to_f32(lv.fresh))
    assert np.array_equal(new_codes, ix.opq.quantize_batch(orc.f16_to_f32(lv.fresh)))   # the device quantiser is the oracle's
    codes2[lv.slots] = new_codes                                # (the rows that stayed keep the codes they were uploaded with)
    tw = lv.twin(mse, rows2, codes2, desc2, h.adj, h.deg, url2)
    assert np.array_equal(lv.vecs.rows(0, ix.n), rows2) and not lv.g.deleted().any()
    qh = lv.fresh[:12].copy()
    qs = orc.f16_to_f32(qh)
    luts = np.stack([ix.opq.preprocess_query(q) for q in qs])
    got = request_calls(mse, lv.view(qh=qh, qs=qs, luts=luts), lv.g)
    want = request_calls(mse, lv.view(searcher=tw.searcher, gcodes=tw.gcodes, qh=qh, qs=qs, luts=luts), tw.g)
    same_answers(got, want)
    with_url, without = set(lv.slots[lv.new_url == 1].tolist()), set(lv.slots[lv.new_url == 0].tolist())
    for name, dp in (("adc", False), ("exact", True)):
        ids, sc, nv, cm, pc = got["topk_" + name]
        found = set(ids[ids != NONE].tolist())
        for i in range(12):
            _, ovids, ovsc, ocm, opc = orc.disk_greedy_search(rows2, h.adj, h.deg, codes2, desc2, int(ix.starts[i]), qh[i], luts[i], SCALES, dp, 2, 64,
                                                             url2)
            wi, ws = sorted_cut(ovids, ovsc, K)
            assert np.array_equal(ids[i], wi) and np.array_equal(sc[i], ws), (name, i)
            assert (int(cm[i]), int(pc[i]), int(nv[i])) == (ocm, opc, len(ovids)), (name, i)
        assert found & with_url, name                           # an inserted row is returned ...
        assert not found & without, name                        # ... and none of those without a url
        print(f"{name}: {len(found & with_url)} inserted ids in the answers; queries that find their own row first: "
              f"{sum(int(ids[i, 0]) == int(lv.slots[i]) for i in range(0, 12, 2))} of 6")
    # the stale state the old recipe left behind would be visible here: the deleted rows' codes differ from the new ones
    assert (ix.codes[lv.slots] != new_codes).any()
    lv.close()
    tw.g.close()


# ---- 3. the norm bound ---------------------------------------------------------------------------------------------------------------
def norm_bits(mse, vl):
    import ctypes as C
    from mse import ffi
    out = (C.c_uint32 * 3)()
    ffi.check(ffi.lib().mse_debug_base_norm_bits(vl._h, out), "debug_base_norm_bits")
    return [int(x) for x in out]


def test_norm_bound_is_raised_never_lowered(world, mse, orc):
    w = world
    f = orc.f16_to_f32(w.fresh)
    small = 0.5 * f
    small[np.abs(small) < 1e-3] = 0                             # half the norm, half the largest component, no subnormal at all
    big = 2.0 * f[:250]
    big[:, :200] = 5e-5                                         # 200 f16 subnormals per row: a subnormal mass of 0.01 ...
    big[:, 200] = 3.0                                           # ... one component of 3, and a norm above 3 (every existing row: norm 1)
    small, big = orc.f16_bits(small[250:]), orc.f16_bits(big)
    vl = mse.VectorList.from_f16s(w.rows, D)
    s = mse.Searcher(vl)
    g = w.deleted_graph(mse, s)
    bits0 = norm_bits(mse, vl)
    assert bits0 == norm_bits(mse, mse.VectorList.from_f16s(w.rows, D))
    g.insert_rows(s, w.slots[250:], small, w.mcfg, w.med)
    assert norm_bits(mse, vl) == bits0                          # smaller rows leave the bound where it was
    g.insert_rows(s, w.slots[:250], big, w.mcfg, w.med)
    rows2 = w.rows.copy()
    rows2[w.slots[250:]], rows2[w.slots[:250]] = small, big
    fresh_bits = norm_bits(mse, mse.VectorList.from_f16s(rows2, D))
    got = norm_bits(mse, vl)
    print(f"bound before {bits0}, after {got}, fresh measurement {fresh_bits}")
    assert got == fresh_bits and all(a > b for a, b in zip(got, bits0))
    # a bound that was never measured stays unmeasured: the first measurement afterwards sees the new rows
    vl2 = mse.VectorList.from_f16s(w.rows, D)
    s2 = mse.Searcher(vl2)
    g2 = w.deleted_graph(mse, s2)
    g2.insert_rows(s2, w.slots[:250], big, w.mcfg, w.med)
    rows3 = w.rows.copy()
    rows3[w.slots[:250]] = big
    assert norm_bits(mse, vl2) == norm_bits(mse, mse.VectorList.from_f16s(rows3, D))
    # the MFMA scan's certificate rests on the bound: queries aimed at the large rows
    q = big[:8]
    ws, wi = orc.bruteforce_topk(rows2, q, K)
    gs, gi = s.bruteforce_topk(q, K, mse.MODE_MFMA)
    assert np.array_equal(gi, wi) and np.array_equal(gs, ws)
    assert set(wi[:, 0].tolist()) <= set(w.slots[:250].tolist())
    g.close()
    g2.close()


# ---- 4. capacity from spare slots ----------------------------------------------------------------------------------------------------
def test_spare_slot_capacity(gpu, mse, orc):
    """An index uploaded with 3 000 slots of which 2 000 are live: the spare ones are marked by delete_rows (no list is rewritten) and
    filled by two inserts of 500; the graph equals the oracle's continued build, and a search for each inserted vector finds its own slot
    first exactly as often as the same search on the oracle's arrays."""
    rows, _ = property_set(orc)
    n, live = len(rows), 2000
    adj0, deg0, med, ocfg = oracle_graph(orc, rows[:live])
    mcfg = mse.IndexBuildConfig(**KW)
    adj, deg = np.zeros((n, 32), np.uint32), np.zeros(n, np.uint32)
    adj[:live], deg[:live] = adj0, deg0
    padded = rows.copy()
    padded[live:] = 0
    vl = mse.VectorList.from_f16s(padded, D)
    s = mse.Searcher(vl)
    g = mse.BuildGraph(n, 32, mse.IndexGraph(adj, deg))
    spare = np.arange(live, n, dtype=np.uint32)
    st = g.delete_rows(s, spare, mcfg)
    assert st["deleted"] == n - live and st["lists_rewritten"] == 0 and g.deleted().sum() == n - live
    wa, wd = adj.copy(), deg.copy()
    now = padded.copy()
    for part in (spare[:500], spare[500:]):
        assert g.insert_rows(s, part, rows[part], mcfg, med, batch=64) == {"inserted": 500, "batches": 8}
        now[part] = rows[part]
        orc.build_graph(now, wa, wd, part, med, ocfg, 64)
        h = g.to_host()
        assert same_graph(h.adj, h.deg, wa, wd)
    assert not g.deleted().any() and np.array_equal(vl.rows(0, n), rows) and (wd[live:] > 0).all()
    found = g.search_batch(s, med, rows[live:], 16)
    mine = sum(int(len(ids) > 0 and ids[0] == live + i) for i, (ids, _, _) in enumerate(found))
    theirs = 0
    for i in range(n - live):
        nb, _ = orc.greedy_search(rows, wa, wd, med, rows[live + i], 16)
        theirs += int(len(nb.ids) > 0 and nb.ids[0] == live + i)
    print(f"inserted vectors that find their own slot at rank 0 (search list 16): {mine} of {n - live} = {mine / (n - live):.4f} (oracle arrays: {theirs})")
    assert mine == theirs and mine > 0
    g.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(index, mse, orc):
    ix = index
    lv = Live(mse, orc, ix, 81)
    h0 = lv.g.to_host()
    rows0 = lv.vecs.rows(0, ix.n)
    tw = lv.twin(mse, ix.base, ix.codes, ix.desc, h0.adj, h0.deg, lv.url_deleted)
    want = request_calls(mse, lv.view(searcher=tw.searcher, gcodes=tw.gcodes), tw.g)
    same_answers(request_calls(mse, lv.view(), lv.g), want)

    def untouched():
        h = lv.g.to_host()
        assert np.array_equal(h.adj, h0.adj) and np.array_equal(h.deg, h0.deg)
        assert np.array_equal(lv.g.deleted(), lv.dead) and np.array_equal(lv.vecs.rows(0, ix.n), rows0)
        same_answers(request_calls(mse, lv.view(), lv.g), want)
    full = dict(quantizer=ix.gpq, codes=lv.gcodes, descriptors=lv.new_desc, has_url=lv.new_url)
    live_row = int(np.flatnonzero(~lv.dead)[7])
    slots = lv.slots

    def bad_slots(i, v):
        a = slots.copy()
        a[i] = v
        return a
    no_desc = mse.Codes(ix.codes)
    short = mse.Codes(ix.codes[:1000], ix.desc[:1000])
    cases = {
        "a live slot": (dict(slots=bad_slots(3, live_row)), "not deleted"),
        "a slot listed twice": (dict(slots=bad_slots(M - 1, slots[0])), "twice"),
        "a slot out of range": (dict(slots=bad_slots(100, ix.n)), "outside"),
        "start deleted": (dict(slots=slots[1:], rows=lv.fresh[1:], descriptors=lv.new_desc[1:], has_url=lv.new_url[1:], start=int(slots[0])), "deleted row"),
        "start among the slots": (dict(start=int(slots[5])), "one of the slots"),
        "start out of range": (dict(start=ix.n), "outside"),
        "codes of another length": (dict(codes=short), "rows"),
        "a quantiser without codes": (dict(codes=None, descriptors=None), "quantiser"),
        "codes without a quantiser": (dict(quantizer=None), "quantiser"),
        "descriptors missing": (dict(descriptors=None), "descriptors"),
        "descriptors superfluous": (dict(codes=no_desc), "descriptors"),
        "descriptors without codes": (dict(quantizer=None, codes=None), "descriptors"),
        "cfg.r above the stride": (dict(config=mse.IndexBuildConfig(r=32, l=64, maxc=250)), "stride"),
        "maxc above the limit": (dict(config=mse.IndexBuildConfig(r=16, l=64, maxc=2000)), "maxc"),
    }
    for name, (kw, match) in cases.items():
        a = dict(slots=slots, rows=lv.fresh, config=lv.mcfg, start=lv.start, batch=64, **full)
        a.update(kw)
        with pytest.raises(mse.MseError, match=match):
            lv.g.insert_rows(lv.searcher, a.pop("slots"), a.pop("rows"), a.pop("config"), a.pop("start"), **a)
        untouched()
    other = mse.Searcher(mse.VectorList.from_f16s(ix.base[:1000], D))
    with pytest.raises(mse.MseError, match="length"):
        lv.g.insert_rows(other, slots, lv.fresh, lv.mcfg, lv.start, **full)
    untouched()
    # ... and the same call without the mistake goes through
    assert lv.g.insert_rows(lv.searcher, slots, lv.fresh, lv.mcfg, lv.start, batch=64, **full)["inserted"] == M
    assert not lv.g.deleted().any()
    with pytest.raises(mse.MseError, match="not deleted"):      # the slots are used up
        lv.g.insert_rows(lv.searcher, slots[:1], lv.fresh[:1], lv.mcfg, lv.start, quantizer=ix.gpq, codes=lv.gcodes, descriptors=lv.new_desc[:1])
    lv.close()
    tw.g.close()


# ---- 6. an insert against requests in flight ------------------------------------------------------------------------------------------
def test_insert_races_the_request_path(index, mse, orc):
    """One insert_rows against 32 threads of one-query disk_query_topk calls through the coalescer and a thread of tickets: every answer
    equals the answer of the index before the insert or after it (which is a fresh upload's) -- no error, no mixed state."""
    ix = index
    lv = Live(mse, orc, ix, 91)
    lv.new_url[:] = 1
    rng = np.random.default_rng(92)
    nq, n_tk = 32, 8
    qh = lv.fresh[:nq].copy()                                   # copies of inserted rows: the answers change with the insert
    q32 = orc.f16_to_f32(lv.fresh[nq:nq + n_tk])
    entries = rng.choice(np.flatnonzero(~lv.dead), 32, replace=False).astype(np.uint32)
    mse.set_entries(lv.g, lv.vecs, entries)

    def ask(graph, searcher, i):
        ids, sc, _ = mse.disk_query_topk(searcher, None, None, graph, qh[i:i + 1], K, None, None, None, True, 2, 48)
        return ids[0].copy(), sc[0].copy()

    def ask32(graph, searcher, i):
        ids, sc, _ = mse.disk_query_topk(searcher, None, None, graph, q32[i:i + 1], K, None, None, None, True, 2, 48)
        return ids[0].copy(), sc[0].copy()
    before = [ask(lv.g, lv.searcher, i) for i in range(nq)]
    before32 = [ask32(lv.g, lv.searcher, i) for i in range(n_tk)]
    answers, tickets, errors = [[] for _ in range(nq)], [[] for _ in range(n_tk)], []
    go, done = threading.Event(), threading.Event()

    def worker(i):
        try:
            go.wait(30)
            for _ in range(5000):
                last = done.is_set()                            # one more whole request after the insert has returned
                answers[i].append(ask(lv.g, lv.searcher, i))
                if last:
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def ticket_worker():
        try:
            tk = mse.QueryTickets(lv.searcher, None, None, lv.g, K, True, 2, 48)
            go.wait(30)
            for _ in range(5000):
                last = done.is_set()
                for i in range(n_tk):
                    tk.submit(q32[i], key=i)
                back = 0
                while back < n_tk:
                    got = tk.collect(timeout_us=20_000_000)
                    assert got, "no ticket came back"
                    for key, t_ids, t_sc in got:
                        tickets[key].append((t_ids[0].copy(), t_sc[0].copy()))
                        back += 1
                if last:
                    break
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(nq)] + [threading.Thread(target=ticket_worker, daemon=True)]
    for t in threads:
        t.start()
    go.set()
    while (min(len(a) for a in answers) < 2 or min(len(a) for a in tickets) < 1) and not errors and any(t.is_alive() for t in threads):
        threading.Event().wait(0.002)
    st = lv.g.insert_rows(lv.searcher, lv.slots, lv.fresh, lv.mcfg, lv.start, quantizer=ix.gpq, codes=lv.gcodes, descriptors=lv.new_desc,
                          has_url=lv.new_url, batch=16)
    done.set()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "a request thread did not come back"
    assert not errors, errors[:3]
    assert st["inserted"] == M
    after = [ask(lv.g, lv.searcher, i) for i in range(nq)]
    after32 = [ask32(lv.g, lv.searcher, i) for i in range(n_tk)]
    # the after-answers are those of a fresh upload of the new arrays
    h = lv.g.to_host()
    rows2, url2 = ix.base.copy(), lv.url_deleted.copy()
    rows2[lv.slots], url2[lv.slots] = lv.fresh, 1
    vl2 = mse.VectorList.from_f16s(rows2, D)
    s2 = mse.Searcher(vl2)
    twin = mse.DeviceGraph(mse.IndexGraph(h.adj, h.deg), url2)
    mse.set_entries(twin, vl2, entries)
    for i in range(nq):
        a = ask(twin, s2, i)
        assert np.array_equal(a[0], after[i][0]) and np.array_equal(a[1], after[i][1]), i
    n_before = n_after = changed = 0
    for i, (got, b, a) in enumerate([(answers[i], before[i], after[i]) for i in range(nq)] + [(tickets[i], before32[i], after32[i]) for i in range(n_tk)]):
        changed += not np.array_equal(b[0], a[0])
        assert not lv.dead[b[0][b[0] != NONE]].any()           # before: no freed slot in an answer
        seen_after = False
        for ids, sc in got:
            is_b = np.array_equal(ids, b[0]) and np.array_equal(sc, b[1])
            is_a = np.array_equal(ids, a[0]) and np.array_equal(sc, a[1])
            assert is_b or is_a, f"query {i}: an answer that is neither the index's before the insert nor its answer after it"
            if is_a and not is_b:
                seen_after = True
            assert not (seen_after and is_b and not is_a), f"query {i}: a before-answer after an after-answer"
            n_before += is_b
            n_after += is_a and not is_b
    print(f"{n_before} answers from the index before the insert, {n_after} from the index after it; {changed} of {nq + n_tk} queries changed their answer")
    assert changed > (nq + n_tk) // 2 and n_before > 0 and n_after > 0
    twin.close()
    lv.close()
