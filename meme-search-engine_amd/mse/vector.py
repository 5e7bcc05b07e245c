"""Host mirror of `diskann::vector` (reference: diskann/src/vector.rs) over the C ABI.

Names, argument meaning and error behaviour follow the Rust module so that tests read like
tests of the reference.  f16 vectors are numpy uint16 arrays of IEEE binary16 bit patterns
(np.float16 arrays are accepted and viewed as bits).  All arithmetic happens on the device.
"""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr

SCALE = 4294967296.0  # vector.rs:46
ID_NONE = 0xFFFFFFFF
GROUP_NONE = 0xFFFFFFFF   # RowGroups: the row is a group of its own

MODE_AUTO, MODE_EXACT, MODE_MFMA = 0, 1, 2
SPARSE_AUTO, SPARSE_OFF, SPARSE_FORCED = 0, 1, 2   # Searcher.set_sparse_maxima


def _bits(a):
    a = np.asarray(a)
    if a.dtype == np.float16:
        a = a.view(np.uint16)
    if a.dtype != np.uint16:
        raise TypeError("f16 vectors must be np.float16 or np.uint16 bit patterns")
    return np.ascontiguousarray(a)


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def scale_dot_result(x):
    """vector.rs:408-411"""
    return int(ffi.lib().mse_scale_dot_f32(float(x)))


def scale_dot_result_f64(x):
    """vector.rs:413-416"""
    return int(ffi.lib().mse_scale_dot_f64(float(x)))


def fast_dot_noprefetch(x, y):
    """vector.rs:255-306.  len % 64 == 0 is required (debug_assert at :259)."""
    x, y = _bits(x).reshape(-1), _bits(y).reshape(-1)
    if x.size != y.size:
        raise MseError("fast_dot: length mismatch")
    out = C.c_int64()
    check(ffi.lib().mse_fast_dot_f16(_p(x, C.c_uint16), _p(y, C.c_uint16), x.size, C.byref(out)), "fast_dot")
    return int(out.value)


def fast_dot(x, y, prefetch=None):
    """vector.rs:192-252: same arithmetic; the third vector is only prefetched."""
    return fast_dot_noprefetch(x, y)


class VectorList:
    """vector.rs:118-186: row-major contiguous f16 rows, here resident in HBM."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keep = keepalive

    @classmethod
    def from_f16s(cls, f16s, d):
        a = _bits(f16s).reshape(-1)
        if a.size % d != 0:
            raise MseError("from_f16s: data length is not a multiple of d")  # assert at vector.rs:174
        n = a.size // d
        return cls(check_ptr(ffi.lib().mse_base_from_host(_p(a, C.c_uint16), n, d), "mse_base_from_host"))

    @classmethod
    def generate(cls, seed, first_row, n_rows, d=1152):
        """Synthetic unit-norm rows made on the device (bit-identical to oracle.gen_rows_f16)."""
        return cls(check_ptr(ffi.lib().mse_base_generate(seed, first_row, n_rows, d), "mse_base_generate"))

    @classmethod
    def wrap_device(cls, dev_ptr, n_rows, d, keepalive=None):
        return cls(check_ptr(ffi.lib().mse_base_wrap_device(dev_ptr, n_rows, d), "mse_base_wrap_device"), keepalive)

    def __len__(self):
        return int(ffi.lib().mse_base_len(self._h))

    @property
    def d_emb(self):
        return int(ffi.lib().mse_base_dim(self._h))

    @property
    def device_ptr(self):
        return ffi.lib().mse_base_device_ptr(self._h)

    def rows(self, first, n):
        out = np.empty((n, self.d_emb), np.uint16)
        check(ffi.lib().mse_base_read_rows(self._h, first, n, _p(out, C.c_uint16)), "mse_base_read_rows")
        return out

    def __getitem__(self, i):
        return self.rows(i, 1)[0]

    def select(self, row_filter):
        """A fresh VectorList holding the rows that `row_filter` (a RowFilter, not longer than this list, on its device) allows, in
        ascending order (mse_base_select): a row gather on the device."""
        if not isinstance(row_filter, RowFilter):
            raise TypeError("row_filter must be a RowFilter")
        return VectorList(check_ptr(ffi.lib().mse_base_select(self._h, row_filter._h), "mse_base_select"))

    def close(self):
        if self._h:
            ffi.lib().mse_base_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowFilter:
    """Allowed-row set of the filtered search (mse_filter): `allowed` is a boolean array of n_rows entries, or an integer array of
    row ids (duplicates allowed; then n_rows is required).  The bitmap lives on the current device and is immutable.  len() is
    n_rows; .count the allowed rows.  Filters are values: a & b, a | b, a ^ b, a - b (and-not), ~a and invert(n_rows) build new ones on
    the device, as do from_descriptors, from_scores and from_device_bits; to_mask() and ids() read one back."""

    def __init__(self, allowed, n_rows=None):
        a = np.asarray(allowed)
        if a.dtype == np.bool_:
            a = a.reshape(-1)
            if n_rows is not None and n_rows != a.size:
                raise ValueError("a boolean filter has one entry per row: n_rows must be its length")
            bits = np.packbits(a, bitorder="little")
            self._h = check_ptr(ffi.lib().mse_filter_from_bits(_p(bits, C.c_uint8), a.size), "mse_filter_from_bits")
        elif np.issubdtype(a.dtype, np.integer):
            if n_rows is None:
                raise ValueError("a filter made from row ids needs n_rows")
            a = a.reshape(-1)
            if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise ValueError("row ids must be in 0 .. 2**32 - 1")
            ids = np.ascontiguousarray(a, np.uint32)
            self._h = check_ptr(ffi.lib().mse_filter_from_ids(_p(ids, C.c_uint32), ids.size, int(n_rows)), "mse_filter_from_ids")
        else:
            raise TypeError("allowed must be a boolean mask or an integer id array")

    @classmethod
    def from_handle(cls, handle):
        """Adopt an mse_filter* made by the library (mse_graph_live_filter): the RowFilter owns and frees it."""
        f = cls.__new__(cls)
        f._h = handle
        return f

    @classmethod
    def wrap(cls, allow):
        """(filter, owned): a RowFilter as it is, anything else made into one (and owned by the caller, to close)."""
        if isinstance(allow, RowFilter):
            return allow, False
        return cls(allow), True

    def __len__(self):
        return int(ffi.lib().mse_filter_len(self._h))

    @property
    def count(self):
        return int(ffi.lib().mse_filter_count(self._h))

    # ---- filters as values: every result is a fresh RowFilter built on the device; the operands stay as they are -------------------

    @classmethod
    def from_descriptors(cls, codes, ranges):
        """The rows of `codes` (a Codes with descriptor bytes) whose descriptor bytes lie in `ranges`: {channel: (lo, hi)}, inclusive;
        channels that are not named are unconstrained (0 .. 255), lo > hi allows nothing.  Reads the bytes as they are in HBM now."""
        nd = int(codes.n_desc)
        lo, hi = np.zeros(max(nd, 1), np.uint8), np.full(max(nd, 1), 255, np.uint8)
        for ch, (a, b) in dict(ranges).items():
            if not 0 <= int(ch) < nd:
                raise ValueError(f"descriptor channel {ch} is not in 0 .. {nd - 1}")
            if not (0 <= int(a) <= 255 and 0 <= int(b) <= 255):
                raise ValueError(f"descriptor bounds must be in 0 .. 255, got ({a}, {b})")
            lo[int(ch)], hi[int(ch)] = int(a), int(b)
        return cls.from_handle(check_ptr(ffi.lib().mse_filter_from_descriptors(codes._h, _p(lo, C.c_uint8), _p(hi, C.c_uint8)),
                                         "mse_filter_from_descriptors"))

    @classmethod
    def from_scores(cls, searcher, query, threshold, within=None):
        """The rows of the searcher's base whose reference-order i64 score against `query` (what Searcher.scores returns) is at least
        `threshold`, and -- with `within`, a RowFilter -- that `within` allows: the range search."""
        if within is not None and not isinstance(within, RowFilter):
            raise TypeError("within must be a RowFilter")
        q = None if query is None else _bits(query).reshape(-1)
        if q is not None and q.size != searcher.vecs.d_emb:
            raise ValueError("the query must have the base's width")
        return cls.from_handle(check_ptr(ffi.lib().mse_filter_from_scores(searcher._h, None if q is None else _p(q, C.c_uint16), int(threshold),
                                                                          None if within is None else within._h), "mse_filter_from_scores"))

    @classmethod
    def from_device_bits(cls, ptr, n_rows):
        """A filter from a packed bitmap that already lives in device memory (`ptr`: its address; (n_rows + 7) // 8 bytes, LSB first,
        as numpy.packbits(..., bitorder="little"); bits past n_rows are ignored)."""
        return cls.from_handle(check_ptr(ffi.lib().mse_filter_from_bits_dev(ptr, int(n_rows)), "mse_filter_from_bits_dev"))

    def slice(self, first_row, n_rows, device=None):
        """Rows first_row .. first_row + n_rows of this filter as a fresh filter over n_rows LOCAL rows (mse_filter_slice): bit r is bit
        first_row + r of self, zero where that is at or past len(self).  first_row need not be a multiple of 32.  device: where the
        result lives (default: with self; another device costs one peer copy of the word range)."""
        if first_row < 0 or n_rows < 0:
            raise ValueError("first_row and n_rows must not be negative")
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_filter_slice(self._h, int(first_row), int(n_rows), -1 if device is None else int(device)),
                                               "mse_filter_slice"))

    @classmethod
    def concat(cls, parts, first_rows, n_rows, device=None):
        """The inverse of slice (mse_filter_concat): a fresh filter over n_rows GLOBAL rows in which parts[i] occupies the rows from
        first_rows[i] on; rows no part covers are excluded.  Parts must not overlap or reach past n_rows."""
        parts = list(parts)
        if len(parts) != len(first_rows):
            raise ValueError("one first row per part")
        if any(not isinstance(p, RowFilter) for p in parts):
            raise TypeError("parts must be RowFilters")
        if n_rows < 0 or any(int(r) < 0 for r in first_rows):
            raise ValueError("rows must not be negative")
        hs = (C.c_void_p * max(len(parts), 1))(*[p._h for p in parts])
        fr = (C.c_uint64 * max(len(parts), 1))(*[int(r) for r in first_rows])
        return cls.from_handle(check_ptr(ffi.lib().mse_filter_concat(hs, fr, len(parts), int(n_rows), -1 if device is None else int(device)),
                                         "mse_filter_concat"))

    def _combine(self, other, op):
        if not isinstance(other, RowFilter):
            return NotImplemented
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_filter_combine(self._h, other._h, op), "mse_filter_combine"))

    def __and__(self, other):
        return self._combine(other, 0)

    def __or__(self, other):
        return self._combine(other, 1)

    def __xor__(self, other):
        return self._combine(other, 2)

    def __sub__(self, other):
        """self AND NOT other"""
        return self._combine(other, 3)

    def invert(self, n_rows=None):
        """NOT self over n_rows rows (default len(self); not fewer): rows at or past len(self) come out allowed."""
        n = len(self) if n_rows is None else int(n_rows)
        if n < 0:
            raise ValueError("n_rows must not be negative")
        if n == 0 and len(self):
            raise MseError("mse_filter_not: n_rows 0 is below the filter's rows")   # 0 means len(self) in the C call
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_filter_not(self._h, n), "mse_filter_not"))

    def __invert__(self):
        return self.invert()

    def to_mask(self):
        """The allowed rows as a boolean array of len(self) entries."""
        n = len(self)
        bits = np.zeros((n + 7) // 8 + 1, np.uint8)   # one spare byte: the call writes exactly (n + 7) // 8
        check(ffi.lib().mse_filter_to_bits(self._h, _p(bits, C.c_uint8)), "mse_filter_to_bits")
        return np.unpackbits(bits[:(n + 7) // 8], count=n, bitorder="little").astype(bool)

    def ids(self, first=0, n=None):
        """The allowed row ids, ascending (uint32): all of them, or n of them from position `first`."""
        n = self.count - int(first) if n is None else int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        out = np.empty(n, np.uint32)
        check(ffi.lib().mse_filter_read_ids(self._h, int(first), n, _p(out, C.c_uint32)), "mse_filter_read_ids")
        return out

    def close(self):
        if self._h:
            ffi.lib().mse_filter_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowGroups:
    """Row grouping of the grouped search (mse_groups): `group_of` is an integer array with one group id per row -- GROUP_NONE (or -1)
    for a row that is a group of its own, any other id below the number of rows.  A grouped search returns one row per group: the
    group's best eligible row in the search's own order (the `seen_videos` walk of src/main.rs:902-917).  The array lives on the current
    device and is immutable.  len() is the number of rows; .count the distinct ids plus the ungrouped rows: the most results a search
    can return.  A grouping may be shorter than what it is used on (later rows are groups of their own), not longer."""

    def __init__(self, group_of):
        self._h = None
        a = np.asarray(group_of)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("group_of must be an integer array: one group id per row")
        if a.ndim != 1:
            raise ValueError("group_of must be one-dimensional: one group id per row")
        if a.size and (a.min() < -1 or a.max() > 0xFFFFFFFF):
            raise ValueError("group ids must be in 0 .. 2**32 - 1 (or -1 for GROUP_NONE)")
        if a.dtype != np.uint32:
            a = np.where(a < 0, GROUP_NONE, a).astype(np.uint32)
        a = np.ascontiguousarray(a)
        self._h = check_ptr(ffi.lib().mse_groups_from_host(_p(a, C.c_uint32), a.size), "mse_groups_from_host")

    @classmethod
    def from_device(cls, ptr, n_rows):
        """mse_groups_from_dev: n_rows u32 group ids that are already in device memory (copied)."""
        g = cls.__new__(cls)
        g._h = check_ptr(ffi.lib().mse_groups_from_dev(ptr, int(n_rows)), "mse_groups_from_dev")
        return g

    @classmethod
    def wrap(cls, groups):
        """(grouping, owned): a RowGroups as it is, anything else made into one (and owned by the caller, to close)."""
        if isinstance(groups, RowGroups):
            return groups, False
        return cls(groups), True

    def __len__(self):
        return int(ffi.lib().mse_groups_len(self._h))

    @property
    def count(self):
        return int(ffi.lib().mse_groups_count(self._h))

    def slice(self, first, n_rows, device=None):
        """mse_groups_slice: a fresh RowGroups over LOCAL rows 0 .. n_rows - 1 with the partition this one has on rows first .. first +
        n_rows - 1, labelled canonically (a grouped row's label is the local id of the first row of its group inside the slice); as long as
        the part of the slice inside this grouping (a slice wholly past it is empty).  device: where it lives (None: this one's)."""
        g = RowGroups.__new__(RowGroups)
        g._h = check_ptr(ffi.lib().mse_groups_slice(self._h, int(first), int(n_rows), -1 if device is None else int(device)), "mse_groups_slice")
        return g

    def to_host(self):
        """The label array as uint32 (GROUP_NONE for ungrouped rows)."""
        out = np.empty(len(self), np.uint32)
        check(ffi.lib().mse_groups_read(self._h, _p(out, C.c_uint32)), "mse_groups_read")
        return out

    def close(self):
        if self._h:
            ffi.lib().mse_groups_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Admission:
    """Result of RowPairs.admit: kept (a RowFilter over the incoming rows: the rows to insert), rep_base (uint32 per incoming row: its
    lowest base partner, ID_NONE without one) and rep_incoming (uint32: the row itself when kept, its lowest kept earlier neighbour in the
    batch when that dropped it, ID_NONE when the base dropped it)."""

    def __init__(self, kept, rep_base, rep_incoming):
        self.kept, self.rep_base, self.rep_incoming = kept, rep_base, rep_incoming

    def close(self):
        if self.kept is not None:
            self.kept.close()
            self.kept = None


class RowPairs:
    """Result of Searcher.near_duplicates (mse_pairs): every pair (lo, hi), lo < hi, of rows of a base whose reference-order i64 score
    reaches the threshold, in canonical order (hi ascending, then lo ascending), each with its exact score.  The list lives on the device
    and is immutable.  len() is the number of rows of the base; .count the pairs.  duplicates(), groups() and representatives() apply the
    keep-first rule (a row is kept iff no kept earlier row forms a pair with it), resolved on the device once per list.
    Searcher.near_duplicates_of gives a CROSS list (kind 1): lo is a row of the resident base, hi a row of the incoming one, len() the
    incoming rows and base_rows the resident ones; its keep-first rule is admit()."""

    def __init__(self, handle):
        self._h = handle

    def __len__(self):
        return int(ffi.lib().mse_pairs_rows(self._h))

    @property
    def kind(self):
        """0: a self list (near_duplicates), 1: a cross list (near_duplicates_of)"""
        return int(ffi.lib().mse_pairs_kind(self._h))

    @property
    def base_rows(self):
        """Rows of the resident base: what lo counts in a cross list; len() for a self list."""
        return int(ffi.lib().mse_pairs_base_rows(self._h))

    def admit(self, among=None):
        """Keep-first continued from the index into the batch (mse_pairs_admit), on a cross list: an incoming row is kept iff it has no
        pair in this list and no kept earlier incoming row pairs with it in `among`, the self list of the incoming rows (None: only the
        base decides).  -> Admission."""
        if among is not None and not isinstance(among, RowPairs):
            raise TypeError("among must be a RowPairs")
        m = len(self)
        rb, ri = np.empty(m, np.uint32), np.empty(m, np.uint32)
        kept = C.c_void_p()
        check(ffi.lib().mse_pairs_admit(self._h, None if among is None else among._h, C.byref(kept), _p(rb, C.c_uint32), _p(ri, C.c_uint32)),
              "mse_pairs_admit")
        return Admission(RowFilter.from_handle(kept.value), rb, ri)

    @property
    def count(self):
        return int(ffi.lib().mse_pairs_count(self._h))

    def read(self, first=0, n=None):
        """(lo uint32, hi uint32, scores int64): all pairs, or n of them from position `first` of the canonical order."""
        n = self.count - int(first) if n is None else int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        lo, hi, sc = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.int64)
        check(ffi.lib().mse_pairs_read(self._h, int(first), n, _p(lo, C.c_uint32), _p(hi, C.c_uint32), _p(sc, C.c_int64)), "mse_pairs_read")
        return lo, hi, sc

    def duplicates(self):
        """The dropped rows as a RowFilter, ready for delete_rows; its complement within the join's `within` is the deduplicated index."""
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_pairs_duplicates(self._h), "mse_pairs_duplicates"))

    def groups(self):
        """A RowGroups: every row of a group of two or more carries its representative's id (the representative included), every other
        row GROUP_NONE."""
        g = RowGroups.__new__(RowGroups)
        g._h = check_ptr(ffi.lib().mse_pairs_groups(self._h), "mse_pairs_groups")
        return g

    def representatives(self):
        """rep (uint32, one per row): the row itself when it is kept, its lowest kept earlier neighbour when it is dropped."""
        out = np.empty(len(self), np.uint32)
        check(ffi.lib().mse_pairs_representatives(self._h, _p(out, C.c_uint32)), "mse_pairs_representatives")
        return out

    def close(self):
        if self._h:
            ffi.lib().mse_pairs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Searcher:
    """Per-thread scratch + stream (reference `Scratch`: lib.rs:157-175, query_disk_index.rs:116-123)."""

    def __init__(self, vecs: VectorList):
        self.vecs = vecs
        self._h = check_ptr(ffi.lib().mse_searcher_new(vecs._h), "mse_searcher_new")

    def set_stream(self, hip_stream):
        check(ffi.lib().mse_searcher_set_stream(self._h, hip_stream), "set_stream")

    def wait_stream(self, producer_stream):
        """Order this searcher's stream after what `producer_stream` (a hipStream_t value) holds now: call it before handing the
        searcher device-resident inputs that another stream wrote."""
        check(ffi.lib().mse_searcher_wait_stream(self._h, producer_stream), "wait_stream")

    def beam_timing(self, enable):
        """Measurement hook of the graph search (mse_searcher_beam_timing): returns what has accumulated so far -- kernel_ms, launches,
        queries, rows_scored (2304-byte row gathers at d = 1152), nodes_fetched (adjacency lists), adc_scored (64-byte code gathers) --
        then sets the switch (0 off, 1 on, 2 on and reset)."""
        out = (C.c_uint64 * 8)()
        check(ffi.lib().mse_searcher_beam_timing(self._h, int(enable), out), "beam_timing")
        return {"kernel_ms": out[0] / 1e3, "launches": int(out[1]), "queries": int(out[2]), "rows_scored": int(out[3]),
                "nodes_fetched": int(out[4]), "adc_scored": int(out[5]), "iterations": int(out[6]), "iterations_replayed": int(out[7])}

    def compact_timing(self, enable):
        """Measurement hook of compact's row-gather kernel (mse_searcher_compact_timing): returns the HIP-event milliseconds of that
        kernel in the last compact made on this searcher while the switch was on (0.0: none), then sets the switch (0 off, 1 on, 2 on
        and reset)."""
        ms = C.c_double()
        check(ffi.lib().mse_searcher_compact_timing(self._h, int(enable), C.byref(ms)), "compact_timing")
        return float(ms.value)

    def bruteforce_topk(self, queries, k, mode=MODE_AUTO, allow=None, groups=None):
        """Brute-force scan + ranking of `evaluate` (query_disk_index.rs:262-273) for a query batch.
        Returns (scores int64 [nq,k], ids uint32 [nq,k]).  allow: a RowFilter or a boolean row mask -- top-k over those rows only.
        groups: a RowGroups or an integer array of group ids -- one result per group, the best (allowed) row of each."""
        d = self.vecs.d_emb
        q = _bits(queries).reshape(-1, d)
        nq = q.shape[0]
        scores = np.empty((nq, k), np.int64)
        ids = np.empty((nq, k), np.uint32)
        if allow is None and groups is None:
            check(ffi.lib().mse_bruteforce_topk_f16(self._h, _p(q, C.c_uint16), nq, k, mode, _p(scores, C.c_int64),
                                                    _p(ids, C.c_uint32)), "bruteforce_topk")
            return scores, ids
        f, owned = RowFilter.wrap(allow) if allow is not None else (None, False)
        g, g_owned = None, False
        try:
            if groups is None:
                check(ffi.lib().mse_bruteforce_topk_filtered_f16(self._h, f._h, _p(q, C.c_uint16), nq, k, mode, _p(scores, C.c_int64),
                                                                 _p(ids, C.c_uint32)), "bruteforce_topk")
            else:
                g, g_owned = RowGroups.wrap(groups)
                check(ffi.lib().mse_bruteforce_topk_grouped_f16(self._h, g._h, f._h if f else None, _p(q, C.c_uint16), nq, k, mode,
                                                                _p(scores, C.c_int64), _p(ids, C.c_uint32)), "bruteforce_topk")
        finally:
            if owned:
                f.close()
            if g_owned:
                g.close()
        return scores, ids

    def bruteforce_topk_dev(self, queries_dev, nq, k, scores_dev, ids_dev, mode=MODE_AUTO, id_offset=0, allow=None, groups=None):
        if allow is None and groups is None:
            check(ffi.lib().mse_bruteforce_topk_f16_dev(self._h, queries_dev, nq, k, mode, id_offset, scores_dev, ids_dev),
                  "bruteforce_topk_dev")
            return
        f, owned = RowFilter.wrap(allow) if allow is not None else (None, False)
        g, g_owned = None, False
        try:
            if groups is None:
                check(ffi.lib().mse_bruteforce_topk_filtered_f16_dev(self._h, f._h, queries_dev, nq, k, mode, id_offset, scores_dev,
                                                                     ids_dev), "bruteforce_topk_dev")
            else:
                g, g_owned = RowGroups.wrap(groups)
                check(ffi.lib().mse_bruteforce_topk_grouped_f16_dev(self._h, g._h, f._h if f else None, queries_dev, nq, k, mode, id_offset,
                                                                    scores_dev, ids_dev), "bruteforce_topk_dev")
            if owned or g_owned:   # the call is asynchronous on the searcher's stream: the filter / grouping must outlive it
                check(ffi.lib().mse_device_synchronize(), "bruteforce_topk_dev")
        finally:
            if owned:
                f.close()
            if g_owned:
                g.close()

    def near_duplicates(self, threshold, window=0, within=None, mode=MODE_AUTO, max_pairs=1 << 32):
        """The near-duplicate self-join of the base (mse_join_self) -> RowPairs: all pairs (lo, hi), lo < hi, hi - lo <= window (0: no
        limit), both rows allowed by `within` (a RowFilter) when given, whose reference-order score is >= threshold.  threshold: an int is
        the i64 score, a float goes through scale_dot_result.  More than max_pairs pairs is an error; join_stats()["kept"] then holds the
        count."""
        if within is not None and not isinstance(within, RowFilter):
            raise TypeError("within must be a RowFilter")
        if isinstance(threshold, (float, np.floating)):
            threshold = scale_dot_result(threshold)
        if window < 0 or max_pairs < 0:
            raise ValueError("window and max_pairs must not be negative")
        return RowPairs(check_ptr(ffi.lib().mse_join_self(self._h, int(threshold), int(window), None if within is None else within._h, int(mode),
                                                          int(max_pairs)), "mse_join_self"))

    def near_duplicates_of(self, incoming, threshold, within=None, mode=MODE_AUTO, max_pairs=1 << 32):
        """The cross join (mse_join_cross) -> RowPairs of kind 1: all pairs (lo, hi) of a row lo of this searcher's base that `within` (a
        RowFilter) allows when given, and a row hi of `incoming`, whose reference-order score is >= threshold.  incoming: a VectorList of
        the base's width on its device, or a numpy array of f16 values / uint16 bits, which is uploaded.  threshold: an int is the i64
        score, a float goes through scale_dot_result.  More than max_pairs pairs is an error; join_stats()["kept"] then holds the
        count."""
        if within is not None and not isinstance(within, RowFilter):
            raise TypeError("within must be a RowFilter")
        if isinstance(threshold, (float, np.floating)):
            threshold = scale_dot_result(threshold)
        if max_pairs < 0:
            raise ValueError("max_pairs must not be negative")
        owned = not isinstance(incoming, VectorList)
        q = VectorList.from_f16s(incoming, self.vecs.d_emb) if owned else incoming
        try:
            return RowPairs(check_ptr(ffi.lib().mse_join_cross(self._h, q._h, int(threshold), None if within is None else within._h, int(mode),
                                                               int(max_pairs)), "mse_join_cross"))
        finally:
            if owned:
                q.close()

    def join_stats(self):
        """Of the last near_duplicates or near_duplicates_of call on this searcher (mse_join_stats); "rounds" is of the last keep-first
        resolution, or admit(), of one of its lists."""
        out = (C.c_uint64 * 6)()
        check(ffi.lib().mse_join_stats(self._h, out), "join_stats")
        return dict(zip(("tiles", "nominated", "rescored", "kept", "strips_repeated", "rounds"), (int(v) for v in out)))

    def join_timing(self, enable):
        """Measurement hook (mse_join_timing): HIP-event milliseconds of the last near_duplicates / near_duplicates_of call made while the switch was on --
        tile launches, re-score launches, building the list -- then sets the switch."""
        out = (C.c_double * 3)()
        check(ffi.lib().mse_join_timing(self._h, int(enable), out), "join_timing")
        return {"tile_ms": out[0], "rescore_ms": out[1], "list_ms": out[2]}

    def debug_join_candidate_capacity(self, n):
        """Test hook: nominated pairs one launch of the join may store (0: the default)."""
        check(ffi.lib().mse_debug_join_candidate_capacity(self._h, int(n)), "debug_join_candidate_capacity")

    def grouped_stats(self):
        """Of the last grouped call on this searcher (mse_searcher_grouped_stats): queries answered from the first candidate prefix,
        from the widened prefix, by the dense path."""
        out = (C.c_uint32 * 3)()
        check(ffi.lib().mse_searcher_grouped_stats(self._h, out), "grouped_stats")
        return tuple(int(v) for v in out)

    def grouped_timing(self, enable):
        """Measurement hook (mse_searcher_grouped_timing): HIP-event milliseconds accumulated so far -- collapse kernel, and of the dense
        passes the score pass, the group atomics, the selection -- then sets the switch (0 off, 1 on, 2 on and reset)."""
        out = (C.c_double * 4)()
        check(ffi.lib().mse_searcher_grouped_timing(self._h, int(enable), out), "grouped_timing")
        return {"collapse_ms": out[0], "dense_score_ms": out[1], "dense_atomics_ms": out[2], "dense_select_ms": out[3]}

    def merge_topk_dev(self, gathered_scores_dev, gathered_ids_dev, n_shards, nq, k, out_scores_dev, out_ids_dev):
        """k-way merge of all-gathered [n_shards][nq][k] shard results (device pointers)."""
        check(ffi.lib().mse_merge_topk_dev(self._h, gathered_scores_dev, gathered_ids_dev, n_shards, nq, k,
                                           out_scores_dev, out_ids_dev), "merge_topk_dev")

    def scores(self, query):
        q = _bits(query).reshape(-1)
        out = np.empty(len(self.vecs), np.int64)
        check(ffi.lib().mse_bruteforce_scores_f16(self._h, _p(q, C.c_uint16), _p(out, C.c_int64)), "bruteforce_scores")
        return out

    def ranks(self, query, ids):
        q = _bits(query).reshape(-1)
        ids = np.ascontiguousarray(ids, np.uint32)
        out = np.empty(ids.size, np.uint32)
        check(ffi.lib().mse_bruteforce_ranks_f16(self._h, _p(q, C.c_uint16), _p(ids, C.c_uint32), ids.size,
                                                 _p(out, C.c_uint32)), "bruteforce_ranks")
        return out

    def score_rows(self, ids, query):
        """out[i] = fast_dot(query, vecs[ids[i]]) (lib.rs:201-207, query_disk_index.rs:168-169)."""
        q = _bits(query).reshape(-1)
        ids = np.ascontiguousarray(ids, np.uint32)
        out = np.empty(ids.size, np.int64)
        check(ffi.lib().mse_score_rows_f16(self._h, _p(ids, C.c_uint32), ids.size, _p(q, C.c_uint16), _p(out, C.c_int64)),
              "score_rows")
        return out

    def scan_timing(self, enable):
        """HIP-event totals of the scan kernel so far -> (total_ms, launches); then set mode
        (0 off, 1 on, 2 on + reset)."""
        ms, n = C.c_double(), C.c_uint64()
        check(ffi.lib().mse_searcher_scan_timing(self._h, enable, C.byref(ms), C.byref(n)), "scan_timing")
        return float(ms.value), int(n.value)

    def last_stats(self):
        a, b = C.c_uint32(), C.c_uint32()
        check(ffi.lib().mse_searcher_last_stats(self._h, C.byref(a), C.byref(b)), "last_stats")
        p, f, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(ffi.lib().mse_searcher_sparse_stats(self._h, C.byref(p), C.byref(f), C.byref(n)), "sparse_stats")
        return {"widened_queries": int(a.value), "max_groups": int(b.value), "sparse_passes": int(p.value),
                "sparse_fallbacks": int(f.value), "sparse_longest_list": int(n.value)}

    def set_sparse_maxima(self, mode="auto", stride=0, capacity=0):
        """Thresholded group maxima of the 320-query pass (include/mse.h mse_searcher_set_sparse_maxima): mode "auto", "off" or
        "forced" (or SPARSE_AUTO / SPARSE_OFF / SPARSE_FORCED); stride and capacity 0 keep their current values."""
        mode = {"auto": SPARSE_AUTO, "off": SPARSE_OFF, "forced": SPARSE_FORCED}.get(mode, mode)
        check(ffi.lib().mse_searcher_set_sparse_maxima(self._h, int(mode), int(stride), int(capacity)), "set_sparse_maxima")

    def close(self):
        if self._h:
            ffi.lib().mse_searcher_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dispatcher:
    """Cross-thread query coalescer over a VectorList (include/mse.h `mse_dispatcher`): the meeting point of the reference's
    one-query-per-request threads (src/main.rs:896-934,1043-1049; src/query_disk_index.rs:711-736).  `search` may be called
    from any number of threads; callers waiting at the same time share one pass over the rows."""

    def __init__(self, vecs: VectorList, max_queries_per_pass=0, max_wait_us=0):
        self.vecs = vecs
        self._h = check_ptr(ffi.lib().mse_dispatcher_new(vecs._h, max_queries_per_pass, max_wait_us), "mse_dispatcher_new")

    def search(self, queries, k, allow=None):
        """allow: a RowFilter -- requests share a pass only with requests of the same filter object."""
        d = self.vecs.d_emb
        q = _bits(queries).reshape(-1, d)
        nq = q.shape[0]
        scores = np.empty((nq, k), np.int64)
        ids = np.empty((nq, k), np.uint32)
        if allow is None:
            check(ffi.lib().mse_dispatcher_topk_f16(self._h, _p(q, C.c_uint16), nq, k, _p(scores, C.c_int64), _p(ids, C.c_uint32)),
                  "dispatcher.search")
            return scores, ids
        f, owned = RowFilter.wrap(allow)
        try:
            check(ffi.lib().mse_dispatcher_topk_filtered_f16(self._h, f._h, _p(q, C.c_uint16), nq, k, _p(scores, C.c_int64),
                                                             _p(ids, C.c_uint32)), "dispatcher.search")
        finally:
            if owned:
                f.close()
        return scores, ids

    def stats(self):
        out = (C.c_uint64 * 6)()
        check(ffi.lib().mse_dispatcher_stats(self._h, out), "dispatcher.stats")
        return dict(zip(("queries", "requests", "passes", "max_pass_queries", "deadline_fires", "retried_alone"), map(int, out)))

    def searcher_handle(self):
        return ffi.lib().mse_dispatcher_searcher(self._h)

    def close(self):
        if self._h:
            ffi.lib().mse_dispatcher_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# mode of the filtered flat scan (MSE_PQ_FILTER_*)
PQ_FILTER_MODES = {"auto": 0, "scan": 1, "list": 2}


class QueryLUT:
    """vector.rs:316-317: chunk-major table [n_chunks][n_centroids] of f32."""

    def __init__(self, table):
        self.table = np.ascontiguousarray(table, np.float32)


class ProductQuantizer:
    """vector.rs:308-406.  Fields as serialised in opq.msgpack (diskann/aopq_train.py:87-93)."""

    def __init__(self, centroids, transform, n_dims_per_code, n_dims):
        centroids = np.ascontiguousarray(centroids, np.float32).reshape(-1)
        transform = np.ascontiguousarray(transform, np.float32).reshape(-1)
        if transform.size != n_dims * n_dims:
            raise MseError("transform must be n_dims x n_dims")  # assert_eq at vector.rs:334
        if centroids.size % n_dims != 0:
            raise MseError("centroids must be rows of n_dims")
        self.n_dims, self.n_dims_per_code = n_dims, n_dims_per_code
        self.n_centroids = centroids.size // n_dims
        self.n_chunks = n_dims // n_dims_per_code
        self._h = check_ptr(ffi.lib().mse_pq_load(_p(centroids, C.c_float), self.n_centroids, _p(transform, C.c_float),
                                                  n_dims, n_dims_per_code), "mse_pq_load")

    @classmethod
    def from_msgpack(cls, blob):
        import msgpack
        m = msgpack.unpackb(blob, raw=False)
        return cls(m["centroids"], m["transform"], m["n_dims_per_code"], m["n_dims"])

    def apply_transform(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.n_dims)
        out = np.empty_like(x)
        check(ffi.lib().mse_pq_apply_transform(self._h, _p(x, C.c_float), x.shape[0], _p(out, C.c_float)),
              "apply_transform")
        return out

    def quantize_batch(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.n_dims)
        codes = np.empty((x.shape[0], self.n_chunks), np.uint8)
        check(ffi.lib().mse_pq_quantize_batch(self._h, _p(x, C.c_float), x.shape[0], _p(codes, C.c_uint8)),
              "quantize_batch")
        return codes

    def preprocess_query(self, query):
        q = np.ascontiguousarray(query, np.float32).reshape(self.n_dims)
        lut = np.empty((self.n_chunks, self.n_centroids), np.float32)
        check(ffi.lib().mse_pq_preprocess_query(self._h, _p(q, C.c_float), _p(lut, C.c_float)), "preprocess_query")
        return QueryLUT(lut)

    def asymmetric_dot_product(self, lut, pq_vectors):
        table = lut.table if isinstance(lut, QueryLUT) else np.ascontiguousarray(lut, np.float32)
        codes = np.ascontiguousarray(pq_vectors, np.uint8).reshape(-1, self.n_chunks)
        out = np.empty(codes.shape[0], np.int64)
        check(ffi.lib().mse_pq_adc(self._h, _p(table, C.c_float), _p(codes, C.c_uint8), codes.shape[0],
                                   _p(out, C.c_int64)), "asymmetric_dot_product")
        return out

    def adc_gather(self, codes, lut, ids, scales=None):
        table = lut.table if isinstance(lut, QueryLUT) else np.ascontiguousarray(lut, np.float32)
        ids = np.ascontiguousarray(ids, np.uint32)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        out = np.empty(ids.size, np.int64)
        check(ffi.lib().mse_pq_adc_gather(self._h, codes._h, _p(table, C.c_float),
                                          _p(sc, C.c_float) if sc is not None else None, _p(ids, C.c_uint32), ids.size,
                                          _p(out, C.c_int64)), "adc_gather")
        return out

    def scan_topk(self, codes, query_f32, r, k, searcher=None, scales=None):
        q = np.ascontiguousarray(query_f32, np.float32).reshape(self.n_dims)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        scores = np.empty(k, np.int64)
        ids = np.empty(k, np.uint32)
        check(ffi.lib().mse_pq_scan_topk(self._h, codes._h, searcher._h if searcher is not None else None,
                                         _p(q, C.c_float), _p(sc, C.c_float) if sc is not None else None, r, k,
                                         _p(scores, C.c_int64), _p(ids, C.c_uint32)), "pq_scan_topk")
        return scores, ids

    def scan_topk_batch(self, codes, queries_f32, r, k, searcher=None, scales=None):
        """scan_topk for [nq, n_dims] queries in one call (one upload, the scans back to back, one download) -> ([nq,k], [nq,k])."""
        q = np.ascontiguousarray(queries_f32, np.float32).reshape(-1, self.n_dims)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        scores = np.empty((q.shape[0], k), np.int64)
        ids = np.empty((q.shape[0], k), np.uint32)
        check(ffi.lib().mse_pq_scan_topk_batch(self._h, codes._h, searcher._h if searcher is not None else None,
                                               _p(q, C.c_float), q.shape[0], _p(sc, C.c_float) if sc is not None else None, r, k,
                                               _p(scores, C.c_int64), _p(ids, C.c_uint32)), "pq_scan_topk_batch")
        return scores, ids

    def scan_topk_filtered(self, codes, allow, query_f32, r, k, searcher=None, scales=None, mode="auto"):
        """scan_topk over the rows `allow` (a RowFilter or a boolean row mask) lets through: exactly scan_topk on codes (and base rows)
        made of the allowed rows alone, ids mapped back.  mode: "auto", "scan" (masked pass over all codes) or "list" (ADC over the
        filter's id list); results are identical."""
        s, i = self.scan_topk_batch_filtered(codes, allow, np.ascontiguousarray(query_f32, np.float32).reshape(1, self.n_dims), r, k,
                                             searcher, scales, mode, _one=True)
        return s[0], i[0]

    def scan_topk_batch_filtered(self, codes, allow, queries_f32, r, k, searcher=None, scales=None, mode="auto", _one=False):
        """scan_topk_batch over the rows `allow` lets through -> ([nq,k], [nq,k]), padded INT64_MIN / 0xFFFFFFFF."""
        q = np.ascontiguousarray(queries_f32, np.float32).reshape(-1, self.n_dims)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        scores = np.empty((q.shape[0], k), np.int64)
        ids = np.empty((q.shape[0], k), np.uint32)
        f, owned = RowFilter.wrap(allow)
        try:
            sh = searcher._h if searcher is not None else None
            scp = _p(sc, C.c_float) if sc is not None else None
            if _one:
                check(ffi.lib().mse_pq_scan_topk_filtered(self._h, codes._h, f._h, sh, _p(q, C.c_float), scp, r, k, PQ_FILTER_MODES[mode],
                                                          _p(scores, C.c_int64), _p(ids, C.c_uint32)), "pq_scan_topk_filtered")
            else:
                check(ffi.lib().mse_pq_scan_topk_batch_filtered(self._h, codes._h, f._h, sh, _p(q, C.c_float), q.shape[0], scp, r, k,
                                                                PQ_FILTER_MODES[mode], _p(scores, C.c_int64), _p(ids, C.c_uint32)),
                      "pq_scan_topk_batch_filtered")
        finally:
            if owned:
                f.close()
        return scores, ids

    @staticmethod
    def filtered_plan(n, allowed, nq):
        """What mode="auto" picks for nq queries over n codes of which `allowed` pass the filter: "scan" or "list" (host only)."""
        m = C.c_int()
        check(ffi.lib().mse_pq_filtered_plan(n, allowed, nq, C.byref(m)), "pq_filtered_plan")
        return {v: name for name, v in PQ_FILTER_MODES.items()}[m.value]

    def debug_group_max_filtered(self, codes, allow, lut0, lut1=None, scales=None):
        """Test hook: debug_group_max through the masked kernels (INT64_MIN for a group without an allowed vector)."""
        ng = (len(codes) + 63) // 64
        l0 = np.ascontiguousarray(lut0, np.float32)
        l1 = None if lut1 is None else np.ascontiguousarray(lut1, np.float32)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        o0 = np.empty(ng, np.int64)
        o1 = np.empty(ng, np.int64) if l1 is not None else None
        f, owned = RowFilter.wrap(allow)
        try:
            check(ffi.lib().mse_debug_pq_group_max_filtered(self._h, codes._h, f._h, _p(l0, C.c_float),
                                                            _p(l1, C.c_float) if l1 is not None else None,
                                                            _p(sc, C.c_float) if sc is not None else None, _p(o0, C.c_int64),
                                                            _p(o1, C.c_int64) if o1 is not None else None), "debug_pq_group_max_filtered")
        finally:
            if owned:
                f.close()
        return (o0, o1) if l1 is not None else o0

    def debug_group_max4_filtered(self, codes, allow, luts, scales=None, n_valid=None, per_pass=4):
        """Test hook: the integer nomination scan through the masked kernels -> (maxima u32 [per_pass, groups], params [per_pass, 4] =
        delta, c, eps, ok); a group without an allowed vector gives the zero-sum key 0."""
        ng = (len(codes) + 63) // 64
        lt = np.ascontiguousarray(luts, np.float32).reshape(per_pass, 64 * 256)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        out = np.zeros((per_pass, ng), np.uint32)
        params = np.zeros((per_pass, 4), np.float64)
        f, owned = RowFilter.wrap(allow)
        try:
            check(ffi.lib().mse_debug_pq4_group_max_filtered(self._h, codes._h, f._h, _p(lt, C.c_float),
                                                             _p(sc, C.c_float) if sc is not None else None,
                                                             per_pass if n_valid is None else n_valid, per_pass, _p(out, C.c_uint32),
                                                             _p(params, C.c_double)), "debug_pq4_group_max_filtered")
        finally:
            if owned:
                f.close()
        return out, params

    def scan_timing(self, enable):
        """HIP-event totals of the four-query scan kernel so far -> (total_ms, launches); then set mode (0 off, 1 on, 2 on + reset)."""
        ms, n = C.c_double(), C.c_uint64()
        check(ffi.lib().mse_pq_scan_timing(self._h, enable, C.byref(ms), C.byref(n)), "pq_scan_timing")
        return float(ms.value), int(n.value)

    def scan_sustained(self):
        """(span_ms, scans) of the batch calls with at least four scans made while timing was on: first scan's start to last scan's
        end -- the back-to-back cost of a pass (reset by scan_timing(2))."""
        ms, n = C.c_double(), C.c_uint64()
        check(ffi.lib().mse_pq_scan_sustained(self._h, C.byref(ms), C.byref(n)), "pq_scan_sustained")
        return float(ms.value), int(n.value)

    @property
    def last_uncertified(self):
        """Queries of the last scan_topk_batch call that the four-query scan could not certify and repeated through the exact scan."""
        return int(ffi.lib().mse_pq_last_uncertified(self._h))

    def debug_group_max(self, codes, lut0, lut1=None, scales=None):
        """Test hook: the flat scan's group maxima (one i64 per 64 vectors) for one table, or for a pair through the
        two-queries-per-pass kernel."""
        ng = (len(codes) + 63) // 64
        l0 = np.ascontiguousarray(lut0, np.float32)
        l1 = None if lut1 is None else np.ascontiguousarray(lut1, np.float32)
        sc = None if scales is None else np.ascontiguousarray(scales, np.float32)
        o0 = np.empty(ng, np.int64)
        o1 = np.empty(ng, np.int64) if l1 is not None else None
        check(ffi.lib().mse_debug_pq_group_max(self._h, codes._h, _p(l0, C.c_float), _p(l1, C.c_float) if l1 is not None else None,
                                               _p(sc, C.c_float) if sc is not None else None, _p(o0, C.c_int64),
                                               _p(o1, C.c_int64) if o1 is not None else None), "debug_pq_group_max")
        return (o0, o1) if l1 is not None else o0

    @classmethod
    def _adopt(cls, handle, n_dims, n_dims_per_code, n_centroids):
        self = cls.__new__(cls)
        self.n_dims, self.n_dims_per_code, self.n_centroids = n_dims, n_dims_per_code, n_centroids
        self.n_chunks = n_dims // n_dims_per_code
        self._h = handle
        return self

    @classmethod
    def train(cls, sample, queries, *, rounds=3, steps=300, lr=5e-4, kmeans_iters=3, seed=4, n_dims_per_code=18, n_centroids=256):
        """The codec as diskann/aopq_train.py:33-85 trains it, on the device (CodecTrainer): a seeded random rotation and k-means, then
        `rounds` x { `steps` Adam steps on the centroids against the query-aware loss; one rotation update }.  sample [n, d] / queries
        [m, d]: float32 host arrays.  -> (ProductQuantizer, info); info carries the first and last loss of every round."""
        sample = np.ascontiguousarray(sample, np.float32)
        tr = CodecTrainer(sample.shape[1], n_dims_per_code, n_centroids)
        try:
            tr.set_sample(sample)
            tr.init(seed)
            tr.set_queries(queries)
            empty = tr.kmeans(kmeans_iters)
            hist = []
            for _ in range(rounds):
                losses = tr.refine(steps, lr=lr)
                if losses:
                    hist += [losses[0], losses[-1]]
                tr.update_rotation()
            info = {"rounds": rounds, "adam_steps_per_round": steps, "lr": lr, "rows": int(sample.shape[0]),
                    "queries": int(np.asarray(queries).shape[0]), "empty_cells_after_kmeans": empty,
                    "query_aware_loss_first_last_per_round": hist}
            return tr.quantizer(), info
        finally:
            tr.close()

    def close(self):
        if self._h:
            ffi.lib().mse_pq_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Codes:
    """PQ codes (+ descriptor bytes) in HBM: index.pq-codes.bin / index.descriptor-codes.bin
    (query_disk_index.rs:686-709)."""

    def __init__(self, codes, descriptors=None):
        codes = np.ascontiguousarray(codes, np.uint8)
        n, cs = codes.shape
        if descriptors is not None:
            descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(n, -1)
            nd = descriptors.shape[1]
            dp = _p(descriptors, C.c_uint8)
        else:
            nd, dp = 0, None
        self._h = check_ptr(ffi.lib().mse_codes_from_host(_p(codes, C.c_uint8), n, cs, dp, nd), "mse_codes_from_host")
        self.code_size, self.n_desc = cs, nd

    @classmethod
    def quantize_base(cls, pq, vecs, descriptors=None):
        """Codes of rows already resident in HBM (mse_codes_quantize_base): quantize_batch over the f32 widenings of the f16 rows,
        on the device -- the encode step of src/dump_processor.rs:468-481."""
        self = cls.__new__(cls)
        if descriptors is not None:
            descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(len(vecs), -1)
            nd, dp = descriptors.shape[1], _p(descriptors, C.c_uint8)
        else:
            nd, dp = 0, None
        self._h = check_ptr(ffi.lib().mse_codes_quantize_base(pq._h, vecs._h, dp, nd), "mse_codes_quantize_base")
        self.code_size, self.n_desc = pq.n_chunks, nd
        return self

    def __len__(self):
        return int(ffi.lib().mse_codes_len(self._h))

    def read_rows(self, first, n, descriptors=False):
        """Entries first .. first + n - 1 as they are in HBM (mse_codes_read_rows): codes [n, code_size] uint8, or with descriptors=True
        (codes, descriptors [n, n_desc])."""
        first, n = int(first), int(n)
        if first < 0 or n < 0 or first + n > len(self):
            raise ValueError("row range out of bounds")
        cs, nd = self.code_size, self.n_desc
        if descriptors and not nd:
            raise MseError("the codes carry no descriptors")
        codes = np.empty((n, cs), np.uint8)
        desc = np.empty((n, nd), np.uint8) if descriptors else None
        check(ffi.lib().mse_codes_read_rows(self._h, first, n, _p(codes, C.c_uint8), _p(desc, C.c_uint8) if descriptors else None),
              "codes_read_rows")
        return (codes, desc) if descriptors else codes

    def describe(self, scores, cdfs, ids=None, first=0, _graph=None):
        """Write the descriptor bytes of scores' rows in place (mse_codes_describe; src/dump_processor.rs:481-491): entry i of `scores`
        (a RowScores) describes row ids[i] (distinct integer ids, one per entry) or row first + i; byte j is the bucket of channel j in
        cdfs[j] (float32 [n_desc, cdf_len], e.g. RowScores.fit_cdfs()), the timestamp channel last.  Other rows keep their bytes.  The
        codes must carry one descriptor byte per channel.  On a live index use DeviceGraph.describe, which takes the graph's lock."""
        c = np.ascontiguousarray(cdfs, np.float32)
        if c.ndim != 2:
            raise MseError("cdfs must be [n_desc, cdf_len]")
        if c.shape[0] != self.n_desc or c.shape[0] != scores.n_desc:
            raise MseError(f"describe: the codes carry {self.n_desc} descriptor bytes per row, the scores have {scores.n_desc} channels "
                           f"and {c.shape[0]} CDFs were given")
        ip = None
        if ids is not None:
            i = np.asarray(ids)
            if i.size and not np.issubdtype(i.dtype, np.integer):
                raise TypeError("ids must be an integer array")
            i = i.reshape(-1)
            if i.size != len(scores):
                raise ValueError(f"ids must name one row per entry of the scores: {i.size} ids for {len(scores)} entries")
            if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
                raise ValueError("ids must be in 0 .. 2**32 - 1")
            i = np.ascontiguousarray(i, np.uint32)
            ip = _p(i, C.c_uint32)
        check(ffi.lib().mse_codes_describe(self._h, _graph, scores._h, ip, int(first), _p(c, C.c_float), c.shape[1]), "codes_describe")

    def close(self):
        if self._h:
            ffi.lib().mse_codes_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def opq_msgpack(centroids, transform, n_dims_per_code, n_dims):
    """The bytes of opq.msgpack (diskann/aopq_train.py:87-93): the four keys with flattened float lists, as ProductQuantizer.from_msgpack
    and the reference's loader read them.  A pure host function."""
    import msgpack
    c = np.ascontiguousarray(centroids, np.float32).reshape(-1)
    t = np.ascontiguousarray(transform, np.float32).reshape(-1)
    if t.size != n_dims * n_dims or c.size % n_dims != 0 or n_dims % n_dims_per_code != 0:
        raise MseError("opq_msgpack: array shapes do not match n_dims / n_dims_per_code")
    return msgpack.packb({"centroids": c.tolist(), "transform": t.tolist(), "n_dims_per_code": int(n_dims_per_code), "n_dims": int(n_dims)})


class CodecTrainer:
    """mse_pq_trainer (include/mse.h): diskann/aopq_train.py:33-85 on the device.  The host keeps the plumbing: seeded choices, the
    random orthonormal start, the queries' second moment and the SVD of the rotation update."""

    def __init__(self, n_dims=1152, n_dims_per_code=18, n_centroids=256):
        self.n_dims, self.n_dims_per_code, self.n_centroids = int(n_dims), int(n_dims_per_code), int(n_centroids)
        self._h = check_ptr(ffi.lib().mse_pq_trainer_new(self.n_dims, self.n_dims_per_code, self.n_centroids), "mse_pq_trainer_new")
        self.n_chunks = self.n_dims // self.n_dims_per_code
        self.n = 0

    def set_sample(self, x_f32):
        x = np.ascontiguousarray(x_f32, np.float32).reshape(-1, self.n_dims)
        check(ffi.lib().mse_pq_trainer_set_sample_f32(self._h, _p(x, C.c_float), x.shape[0]), "pq_trainer_set_sample_f32")
        self.n = x.shape[0]

    def set_sample_rows(self, vector_list_or_searcher, ids):
        """Rows `ids` of a resident index as the sample: gathered and widened on the device, nothing crosses PCIe but the ids."""
        vecs = getattr(vector_list_or_searcher, "vecs", vector_list_or_searcher)
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        check(ffi.lib().mse_pq_trainer_set_sample_base(self._h, vecs._h, _p(ids, C.c_uint32), ids.size), "pq_trainer_set_sample_base")
        self.n = ids.size      # (the rows are copied: the index need not outlive the call)

    def set_transform(self, T):
        T = np.ascontiguousarray(T, np.float32).reshape(self.n_dims, self.n_dims)
        check(ffi.lib().mse_pq_trainer_set_transform(self._h, _p(T, C.c_float)), "pq_trainer_set_transform")

    def set_centroids(self, centroids):
        c = np.ascontiguousarray(centroids, np.float32).reshape(self.n_centroids, self.n_dims)
        check(ffi.lib().mse_pq_trainer_set_centroids(self._h, _p(c, C.c_float)), "pq_trainer_set_centroids")

    def set_query_moment(self, C0):
        m = np.ascontiguousarray(C0, np.float32).reshape(self.n_dims, self.n_dims)
        check(ffi.lib().mse_pq_trainer_set_query_moment(self._h, _p(m, C.c_float)), "pq_trainer_set_query_moment")

    def init(self, seed):
        """aopq_train.py:62-73: a random orthonormal transform (numpy QR), centroids = the rotated rows at n_centroids seeded distinct ids."""
        if not self.n:
            raise MseError("CodecTrainer.init: set a sample first")
        rng = np.random.default_rng(seed)
        T = np.linalg.qr(rng.standard_normal((self.n_dims, self.n_dims)))[0].astype(np.float32)
        rows = np.sort(rng.choice(self.n, self.n_centroids, replace=False))
        self.set_transform(T)
        self.set_centroids(self.rotated_rows(rows))
        return rows

    def rotated_rows(self, rows):
        """X'[rows]: the listed sample rows under the current transform."""
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1)
        out = np.empty((rows.size, self.n_dims), np.float32)
        check(ffi.lib().mse_pq_trainer_rotated_rows(self._h, _p(rows, C.c_uint32), rows.size, _p(out, C.c_float)), "pq_trainer_rotated_rows")
        return out

    def set_queries(self, q_f32):
        """C0 = Q^T Q / m of the unrotated queries, in float64 on the host, handed over as f32."""
        q = np.ascontiguousarray(q_f32, np.float64).reshape(-1, self.n_dims)
        self.set_query_moment((q.T @ q / q.shape[0]).astype(np.float32))

    def kmeans(self, iters):
        empty = C.c_uint64(0)
        check(ffi.lib().mse_pq_trainer_kmeans(self._h, int(iters), C.byref(empty)), "pq_trainer_kmeans")
        return int(empty.value)

    def refine(self, steps, lr=5e-4, betas=(0.9, 0.999), eps=1e-8):
        loss = np.zeros(max(int(steps), 1), np.float64)
        check(ffi.lib().mse_pq_trainer_refine(self._h, int(steps), lr, betas[0], betas[1], eps, _p(loss, C.c_double)), "pq_trainer_refine")
        return [float(v) for v in loss[:int(steps)]]

    def loss(self):
        out = C.c_double(0.0)
        check(ffi.lib().mse_pq_trainer_loss(self._h, C.byref(out)), "pq_trainer_loss")
        return float(out.value)

    def cross(self):
        M = np.empty((self.n_dims, self.n_dims), np.float64)
        check(ffi.lib().mse_pq_trainer_cross(self._h, _p(M, C.c_double)), "pq_trainer_cross")
        return M

    def update_rotation(self):
        """aopq_train.py:79-85: U S V^T = svd(X'^T Y) in float64, T_new = (U V^T)^T T_old.  The centroids are not refitted."""
        u, _, vt = np.linalg.svd(self.cross())
        T_old = self.arrays()[1].astype(np.float64)
        self.set_transform(((u @ vt).T @ T_old).astype(np.float32))

    def arrays(self):
        c = np.empty((self.n_centroids, self.n_dims), np.float32)
        T = np.empty((self.n_dims, self.n_dims), np.float32)
        check(ffi.lib().mse_pq_trainer_read(self._h, _p(c, C.c_float), _p(T, C.c_float)), "pq_trainer_read")
        return c, T

    def codes(self):
        out = np.empty((self.n, self.n_chunks), np.uint8)
        check(ffi.lib().mse_pq_trainer_codes(self._h, _p(out, C.c_uint8)), "pq_trainer_codes")
        return out

    def adam_state(self):
        m = np.empty((self.n_centroids, self.n_dims), np.float32)
        v = np.empty_like(m)
        t = C.c_uint64(0)
        check(ffi.lib().mse_pq_trainer_adam_state(self._h, _p(m, C.c_float), _p(v, C.c_float), C.byref(t)), "pq_trainer_adam_state")
        return m, v, int(t.value)

    def set_adam_state(self, m, v, t):
        m = np.ascontiguousarray(m, np.float32).reshape(self.n_centroids, self.n_dims)
        v = np.ascontiguousarray(v, np.float32).reshape(self.n_centroids, self.n_dims)
        check(ffi.lib().mse_pq_trainer_set_adam_state(self._h, _p(m, C.c_float), _p(v, C.c_float), int(t)), "pq_trainer_set_adam_state")

    def gradient(self):
        """The gradient the last refine step applied, [n_centroids, n_dims]."""
        g = np.empty((self.n_centroids, self.n_dims), np.float32)
        check(ffi.lib().mse_pq_trainer_gradient(self._h, _p(g, C.c_float)), "pq_trainer_gradient")
        return g

    def timing(self):
        """HIP-event milliseconds of the last refine step: {assign, gemm, accumulate, adam}."""
        ms = np.zeros(4, np.float32)
        check(ffi.lib().mse_pq_trainer_timing(self._h, _p(ms, C.c_float)), "pq_trainer_timing")
        return dict(zip(("assign", "gemm", "accumulate", "adam"), (float(x) for x in ms)))

    def quantizer(self):
        h = check_ptr(ffi.lib().mse_pq_trainer_finish(self._h), "mse_pq_trainer_finish")
        return ProductQuantizer._adopt(h, self.n_dims, self.n_dims_per_code, self.n_centroids)

    def close(self):
        if self._h:
            ffi.lib().mse_pq_trainer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def descriptor_product(scales, descriptors, idx):
    """query_disk_index.rs:135-142"""
    s = np.ascontiguousarray(scales, np.float32)
    d = np.ascontiguousarray(descriptors, np.uint8)
    return int(ffi.lib().mse_descriptor_product(_p(s, C.c_float), s.size, _p(d, C.c_uint8), int(idx)))
