"""The shard partition (include/mse.h mse_partitioner): kmeans.py's balanced shard centroids, the spill-2 assignment of
src/dump_processor.rs:438-461 and the per-shard medioids, on the device.  All arithmetic happens in libmse_hip.so."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr
from .vector import RowFilter, VectorList, _bits, _p

CODE_REJECTED, CODE_ACCEPTED, CODE_REROLLED = 0, 1, 2
_CONFIG_KEYS = ("temperature0", "accept_decay", "reject_decay", "reroll_heat", "temperature_cap", "reroll_after", "seed", "stop_fraction")


def medioid_ids(vecs, ids):
    """mse_medioid_ids: the position in `ids` of the medioid (diskann/src/lib.rs:52-68) of vecs' rows ids, in list order."""
    ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), np.uint32)
    out = C.c_uint32()
    check(ffi.lib().mse_medioid_ids(vecs._h, _p(ids, C.c_uint32), ids.size, C.byref(out)), "mse_medioid_ids")
    return int(out.value)


def _widen_f16(bits):
    return _bits(bits).view(np.float16).astype(np.float32)


class ShardPartitioner:
    """ShardPartitioner(n_shards, d=1152, **config): config takes the fields of mse_partition_config (the script's values by default).
    set_sample -> anneal -> assign -> assignment / counts / shard_filter / members / entries."""

    def __init__(self, n_shards, d=1152, **config):
        unknown = set(config) - set(_CONFIG_KEYS)
        if unknown:
            raise TypeError("unknown annealing parameters: " + ", ".join(sorted(unknown)))
        cfg = ffi.PartitionConfig()
        ffi.lib().mse_partition_config_default(C.byref(cfg))
        for k, v in config.items():
            setattr(cfg, k, v)
        self.n_shards, self.d, self.config = int(n_shards), int(d), cfg
        self._h = check_ptr(ffi.lib().mse_partition_new(self.n_shards, self.d, C.byref(cfg)), "mse_partition_new")

    # ---- the sample and the annealing -------------------------------------------------------------------------------------------
    def set_sample(self, rows, ids=None):
        """rows: f16 rows [n][d], or a VectorList with the ids of its rows to take (also as one (vecs, ids) pair)."""
        if isinstance(rows, tuple):
            rows, ids = rows
        if isinstance(rows, VectorList):
            if ids is None:
                raise TypeError("a sample from a resident base needs the row ids")
            ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), np.uint32)
            check(ffi.lib().mse_partition_set_sample_base(self._h, rows._h, _p(ids, C.c_uint32), ids.size), "mse_partition_set_sample_base")
            self._n = ids.size
        else:
            a = _bits(rows).reshape(-1, self.d)
            check(ffi.lib().mse_partition_set_sample_f16(self._h, _p(a, C.c_uint16), a.shape[0]), "mse_partition_set_sample_f16")
            self._n = a.shape[0]
        return self

    def anneal(self, iters):
        """iters more iterations; returns their trace (F uint64, code uint8), shorter when the run stopped."""
        before = self.state().t
        check(ffi.lib().mse_partition_anneal(self._h, int(iters)), "mse_partition_anneal")
        self._acen = None      # the assignment's centroids are now the annealed f16 result widened
        return self.trace(before)

    def state(self):
        st = ffi.PartitionState()
        check(ffi.lib().mse_partition_state(self._h, C.byref(st)), "mse_partition_state")
        return st

    def trace(self, first=0, n=None):
        n = self.state().t - int(first) if n is None else int(n)
        F, code = np.empty(n, np.uint64), np.empty(n, np.uint8)
        check(ffi.lib().mse_partition_trace(self._h, int(first), n, _p(F, C.c_uint64), _p(code, C.c_uint8)), "mse_partition_trace")
        return F, code

    def _read(self, which):
        out = np.empty((self.n_shards, self.d), np.uint16 if which == 2 else np.float32)
        args = [None, None, None]
        args[which] = _p(out, C.c_uint16 if which == 2 else C.c_float)
        check(ffi.lib().mse_partition_centroids(self._h, *args), "mse_partition_centroids")
        return out

    def raw_centroids(self):
        return self._read(0)

    def centroids(self):
        """The annealed centroids, normalised (kmeans.py:127), float32."""
        return self._read(1)

    def centroids_f16(self):
        """The bytes of centroids.bin (kmeans.py:153), as uint16 bit patterns."""
        return self._read(2)

    def set_centroids(self, c):
        """The assignment's centroids: f16 (bit patterns or np.float16; widened as the reference decodes the file) or float32, used as given."""
        c = np.asarray(c)
        c = np.ascontiguousarray(c, np.float32) if c.dtype == np.float32 else _widen_f16(c)
        c = np.ascontiguousarray(c.reshape(self.n_shards, self.d))
        check(ffi.lib().mse_partition_set_centroids(self._h, _p(c, C.c_float)), "mse_partition_set_centroids")
        self._acen = c
        return self

    # ---- the two forms of the pass, over the sample ------------------------------------------------------------------------------
    def count(self, centroids, top2=False):
        c = np.ascontiguousarray(np.asarray(centroids, np.float32).reshape(self.n_shards, self.d))
        sizes = np.empty((2, self.n_shards), np.uint64)
        t2 = np.empty((self._n_sample(), 2), np.uint8) if top2 else None
        check(ffi.lib().mse_partition_count(self._h, _p(c, C.c_float), _p(sizes, C.c_uint64), _p(t2, C.c_uint8) if top2 else None), "mse_partition_count")
        return (sizes, t2) if top2 else sizes

    def scores(self, centroids):
        c = np.ascontiguousarray(np.asarray(centroids, np.float32).reshape(self.n_shards, self.d))
        out = np.empty((self._n_sample(), self.n_shards), np.float64)
        check(ffi.lib().mse_partition_scores(self._h, _p(c, C.c_float), _p(out, C.c_double)), "mse_partition_scores")
        return out

    def _n_sample(self):
        n = getattr(self, "_n", None)
        if n is None:
            raise MseError("no sample set")
        return n

    # ---- the assignment --------------------------------------------------------------------------------------------------------
    def assign(self, rows, fudge=0.2, first=0, n=None):
        """Append rows to the assignment: f16 rows [n][d], or rows first .. first + n of a VectorList (all of it by default)."""
        if isinstance(rows, VectorList):
            n = len(rows) - int(first) if n is None else int(n)
            check(ffi.lib().mse_partition_assign_base(self._h, rows._h, int(first), n, float(fudge)), "mse_partition_assign_base")
        else:
            a = _bits(rows).reshape(-1, self.d)
            check(ffi.lib().mse_partition_assign_f16(self._h, _p(a, C.c_uint16), a.shape[0], float(fudge)), "mse_partition_assign_f16")
        return self

    def reset_assignment(self):
        check(ffi.lib().mse_partition_assign_reset(self._h), "mse_partition_assign_reset")
        return self

    def n_assigned(self):
        n = C.c_uint64()
        check(ffi.lib().mse_partition_counts(self._h, None, C.byref(n)), "mse_partition_counts")
        return int(n.value)

    def assignment(self):
        out = np.empty((self.n_assigned(), 2), np.uint8)
        check(ffi.lib().mse_partition_assignment(self._h, 0, out.shape[0], _p(out, C.c_uint8)), "mse_partition_assignment")
        return out

    def counts(self):
        out = np.empty(self.n_shards, np.uint64)
        check(ffi.lib().mse_partition_counts(self._h, _p(out, C.c_uint64), None), "mse_partition_counts")
        return out

    def shard_filter(self, s):
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_partition_shard_filter(self._h, int(s)), "mse_partition_shard_filter"))

    def members(self, s):
        """Row ids of shard s, ascending: the order the reference appends them to the shard file."""
        f = self.shard_filter(s)
        try:
            return f.ids()
        finally:
            f.close()

    def entries(self, vecs):
        """(centroids f32 [S][d], node_ids u32 [S]) for set_entry_centroids: the assignment's centroids and each shard's medioid among
        the assigned rows of vecs."""
        cen = getattr(self, "_acen", None)
        if cen is None:
            cen = _widen_f16(self.centroids_f16())
        node_ids = np.empty(self.n_shards, np.uint32)
        for s in range(self.n_shards):
            m = self.members(s)
            if m.size == 0:
                raise MseError(f"shard {s} has no rows")
            node_ids[s] = m[medioid_ids(vecs, m)]
        return cen, node_ids

    def timing(self):
        ms = np.zeros(3, np.float32)
        check(ffi.lib().mse_partition_timing(self._h, _p(ms, C.c_float)), "mse_partition_timing")
        return ms

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_partition_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
