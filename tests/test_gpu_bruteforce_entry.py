"""The brute-force entry points as one table: mse_bruteforce_topk_f16, _f16_dev, _filtered_f16 and _filtered_f16_dev share one body
(bruteforce.hip), and so do the shard group's four (shard_group.hip).  Every cell of (query count x mode x host / device form x filter)
equals the oracle over the allowed rows bit for bit, and every entry point validates its arguments in one order and writes nothing when
it refuses a call."""
import ctypes as C

import numpy as np
import pytest

from conftest import SEED_BASE, SEED_QUERY

pytestmark = pytest.mark.gpu
D = 1152
N = 4099            # no multiple of 32, 64 or 256
K = 10
NQS = [1, 8, 9, 321]   # 1: through the coalescer; 8 | 9: the two sides of the direct AUTO rule; 321: more than one 320-query tile
MODES = {"auto": 0, "exact": 1, "mfma": 2}
FILTERS = ["none", "all", "half", "1%"]
ID_OFFSET = 1_000_003
ID_NONE = 0xFFFFFFFF
SENTINEL = 7


def _masks():
    rng = np.random.default_rng(0xB7)
    return {"none": None, "all": np.ones(N, bool), "half": rng.random(N) < 0.5, "1%": rng.random(N) < 0.01}


class Table:
    """The base, the queries, the filters and the oracle's answers, made once for the module."""

    def __init__(self, mse, orc):
        self.base = orc.gen_rows_f16(SEED_BASE, 0, N)
        self.q = np.ascontiguousarray(orc.gen_rows_f16(SEED_QUERY, 0, max(NQS)))
        self.vecs = mse.VectorList.from_f16s(self.base, D)
        self.searcher = mse.Searcher(self.vecs)
        self.masks = _masks()
        self.filters = {name: None if m is None else mse.RowFilter(m) for name, m in self.masks.items()}
        self.want = {}
        for name, m in self.masks.items():
            allowed = np.arange(N) if m is None else np.flatnonzero(m)
            assert allowed.size >= K
            ws, wi = orc.bruteforce_topk(self.base[allowed], self.q, K)
            self.want[name] = (ws, allowed[wi].astype(np.uint32))


@pytest.fixture(scope="module")
def table(gpu, mse, orc):
    return Table(mse, orc)


def test_masks_lie_on_both_sides_of_the_crossover(table):
    # filter_sparse at 9 queries: count x ceil(9 / 8) x 3 <= n x ceil(9 / 320) x 2, i.e. count <= n / 3
    assert table.masks["1%"].sum() * 2 * 3 <= N * 2 < table.masks["half"].sum() * 2 * 3
    assert np.array_equal(table.want["all"][0], table.want["none"][0]) and np.array_equal(table.want["all"][1], table.want["none"][1])


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("nq", NQS)
def test_host_form_equals_oracle(table, mse, nq, mode, flt):
    ws, wi = table.want[flt]
    sc, ids = table.searcher.bruteforce_topk(table.q[:nq], K, MODES[mode], allow=table.filters[flt])
    assert np.array_equal(ids, wi[:nq]) and np.array_equal(sc, ws[:nq])


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("nq", NQS)
def test_device_form_equals_oracle(table, mse, nq, mode, flt):
    import torch
    ws, wi = table.want[flt]
    qd = torch.from_numpy(table.q[:nq].view(np.int16)).cuda()
    sd = torch.full((nq, K), SENTINEL, dtype=torch.int64, device="cuda")
    idd = torch.full((nq, K), SENTINEL, dtype=torch.int32, device="cuda")
    table.searcher.bruteforce_topk_dev(qd.data_ptr(), nq, K, sd.data_ptr(), idd.data_ptr(), MODES[mode], ID_OFFSET, allow=table.filters[flt])
    mse.ffi.check(mse.ffi.lib().mse_device_synchronize())
    assert np.array_equal(idd.cpu().numpy().view(np.uint32), wi[:nq] + np.uint32(ID_OFFSET))
    assert np.array_equal(sd.cpu().numpy(), ws[:nq])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("nq", NQS)
def test_all_rows_filter_equals_unfiltered(table, mse, nq, mode):
    us, ui = table.searcher.bruteforce_topk(table.q[:nq], K, MODES[mode])
    fs, fi = table.searcher.bruteforce_topk(table.q[:nq], K, MODES[mode], allow=table.filters["all"])
    assert np.array_equal(ui, fi) and np.array_equal(us, fs)


# ---- validation: one order for every entry point, and a refused call writes nothing -------------------------------------------------

ENTRIES = {   # name -> (library function, takes a filter, device form, takes an id offset)
    "topk": ("mse_bruteforce_topk_f16", False, False, False),
    "topk_filtered": ("mse_bruteforce_topk_filtered_f16", True, False, False),
    "topk_dev": ("mse_bruteforce_topk_f16_dev", False, True, True),
    "topk_filtered_dev": ("mse_bruteforce_topk_filtered_f16_dev", True, True, True),
    "group": ("mse_shard_group_search", False, False, False),
    "group_filtered": ("mse_shard_group_search_filtered", True, False, False),
    "group_dev": ("mse_shard_group_search_dev", False, True, False),
    "group_filtered_dev": ("mse_shard_group_search_filtered_dev", True, True, False),
}


class Outputs:
    """[3][2000] scores and ids pre-filled with a sentinel, on the host or the device, and the three queries beside them."""

    def __init__(self, q, device):
        self.device = device
        if device:
            import torch
            self.qd = torch.from_numpy(q.view(np.int16)).cuda()
            self.sc = torch.full((3, 2000), SENTINEL, dtype=torch.int64, device="cuda")
            self.ids = torch.full((3, 2000), SENTINEL, dtype=torch.int32, device="cuda")
            self.args = (self.qd.data_ptr(), self.sc.data_ptr(), self.ids.data_ptr())
        else:
            self.q = q
            self.sc = np.full((3, 2000), SENTINEL, np.int64)
            self.ids = np.full((3, 2000), SENTINEL, np.uint32)
            self.args = (q.ctypes.data_as(C.POINTER(C.c_uint16)), self.sc.ctypes.data_as(C.POINTER(C.c_int64)),
                         self.ids.ctypes.data_as(C.POINTER(C.c_uint32)))

    def untouched(self, mse):
        if self.device:
            mse.ffi.check(mse.ffi.lib().mse_device_synchronize())
            return bool((self.sc == SENTINEL).all()) and bool((self.ids == SENTINEL).all())
        return bool((self.sc == SENTINEL).all() and (self.ids == SENTINEL).all())


def call(mse, entry, handle, flt, out, nq, k, mode):
    fn, filtered, _, offset = ENTRIES[entry]
    qp, sp, ip = out.args
    args = [handle] + ([flt] if filtered else []) + [qp, nq, k, mode] + ([0] if offset else []) + [sp, ip]
    return getattr(mse.ffi.lib(), fn)(*args)


@pytest.fixture(scope="module")
def handles(table, mse):
    """entry -> (handle, filter handle or None, what a null handle is called)"""
    group = mse.ShardGroup(1, D)
    group.load_host(table.base)
    sf = group.filter(table.filters["all"])
    out = {}
    for entry, (_, filtered, _, _) in ENTRIES.items():
        if entry.startswith("group"):
            out[entry] = (group._h, sf._h if filtered else None, b"null shard group")
        else:
            out[entry] = (table.searcher._h, table.filters["all"]._h if filtered else None, b"null searcher")
    yield out
    sf.close()
    group.close()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_validation(table, handles, mse, entry):
    lib = mse.ffi.lib()
    h, f, null_text = handles[entry]
    out = Outputs(table.q[:3], ENTRIES[entry][2])
    assert call(mse, entry, None, f, out, 3, K, 0) == -1 and null_text in lib.mse_last_error()
    assert call(mse, entry, h, f, out, 3, 1985, 0) == -1 and b"k too large (max 1984)" in lib.mse_last_error()
    assert call(mse, entry, h, f, out, 3, K, 7) == -1 and b"unknown mode" in lib.mse_last_error()
    assert call(mse, entry, h, f, out, 0, K, 0) == 0
    assert call(mse, entry, h, f, out, 3, 0, 0) == 0
    if ENTRIES[entry][1]:   # a missing filter is reported before the arguments are looked at
        assert call(mse, entry, h, None, out, 3, 1985, 7) == -1 and b"null" in lib.mse_last_error() and b"filter" in lib.mse_last_error()
    assert out.untouched(mse)


@pytest.mark.parametrize("entry", ["topk", "topk_filtered", "topk_dev", "topk_filtered_dev"])
def test_unknown_mode_on_an_empty_base_is_an_error(gpu, mse, orc, entry):
    lib = mse.ffi.lib()
    vecs = mse.VectorList.from_f16s(np.zeros((0, D), np.uint16), D)
    s = mse.Searcher(vecs)
    f = mse.RowFilter(np.zeros(0, bool)) if ENTRIES[entry][1] else None
    out = Outputs(np.ascontiguousarray(orc.gen_rows_f16(SEED_QUERY, 0, 3)), ENTRIES[entry][2])
    assert call(mse, entry, s._h, None if f is None else f._h, out, 3, K, 7) == -1 and b"unknown mode" in lib.mse_last_error()
    assert out.untouched(mse)
    s.close()
    vecs.close()
