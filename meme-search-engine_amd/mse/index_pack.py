"""Host mirror of the index-packing pieces of dump_processor: ScoreModel (src/score_model.rs) and the CDF inversion that
turns score channels into descriptor bytes (src/dump_processor.rs:483-491).  quantize_batch lives on ProductQuantizer.
Over a resident index the same runs without the rows leaving the device: ScoreModel.score_rows -> RowScores (scores, order statistics,
the CDF fit of meme-rater/compute_cdf.py:64-71) -> Codes.describe / DeviceGraph.describe."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr
from .vector import _bits, _p


class ScoreModel:
    """src/score_model.rs:4-49.  Tensors as stored in model.safetensors: up_proj [d_hidden, d_emb], bias [d_hidden],
    down_proj [output_channels, d_hidden]."""

    def __init__(self, up_proj, bias, down_proj):
        up = np.ascontiguousarray(up_proj, np.float32)
        b = np.ascontiguousarray(bias, np.float32).reshape(-1)
        down = np.ascontiguousarray(down_proj, np.float32)
        if up.ndim != 2 or down.ndim != 2 or up.shape[0] != b.size or down.shape[1] != b.size:
            raise MseError("score model: inconsistent tensor shapes")
        self.d_emb, self.d_hidden, self.output_channels = up.shape[1], up.shape[0], down.shape[0]
        self._h = check_ptr(ffi.lib().mse_score_model_load(_p(up, C.c_float), _p(b, C.c_float), _p(down, C.c_float), self.d_emb,
                                                           self.d_hidden, self.output_channels), "mse_score_model_load")

    @classmethod
    def load(cls, path):
        from safetensors.numpy import load_file
        t = load_file(path)
        return cls(t["up_proj"], t["bias"], t["down_proj"])

    def score_batch(self, x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.d_emb)
        out = np.empty((x.shape[0], self.output_channels), np.float32)
        check(ffi.lib().mse_score_model_score_batch(self._h, _p(x, C.c_float), x.shape[0], _p(out, C.c_float)), "score_batch")
        return out

    def score_rows(self, vecs_or_searcher, ids=None, first=0, n=None, timestamps=None):
        """score_batch over rows resident in HBM (mse_scores_from_base), on the f32 matrix cores: rows `ids` (any order, repeats allowed)
        or first .. first + n (n None: to the end) of a VectorList or of a Searcher's rows.  A 2-D numpy array of f16 rows (np.float16 or
        uint16 bits, any width) is uploaded for the call and scored by the same kernel (mse_scores_from_f16).  timestamps: one integer
        in [0, 2**32) per row, the extra channel.  A row's scores are the same bits however it is asked for.  Returns a RowScores (on
        the device)."""
        host = None
        if isinstance(vecs_or_searcher, np.ndarray):
            host = _bits(vecs_or_searcher)
            if host.ndim != 2:
                raise MseError("score_rows: host rows must be [n_rows, d]")
            vecs = host
        else:
            vecs = getattr(vecs_or_searcher, "vecs", vecs_or_searcher)
            if getattr(vecs, "_h", None) is None:
                raise MseError("score_rows needs a VectorList, a Searcher over one, or a 2-D array of f16 rows")
        ip = None
        if ids is not None:
            i = np.asarray(ids)
            if i.size and not np.issubdtype(i.dtype, np.integer):
                raise TypeError("ids must be an integer array")
            i = i.reshape(-1)
            if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
                raise ValueError("ids must be in 0 .. 2**32 - 1")
            i = np.ascontiguousarray(i, np.uint32)
            ip, count, first = _p(i, C.c_uint32), i.size, 0
        else:
            first = int(first)
            count = len(vecs) - first if n is None else int(n)
            if first < 0 or count < 0:
                raise ValueError("row range out of bounds")
        ts, tp = _timestamps(timestamps, count)
        if host is not None:
            h = check_ptr(ffi.lib().mse_scores_from_f16(self._h, _p(host, C.c_uint16), host.shape[0], host.shape[1], ip, first, count, tp),
                          "mse_scores_from_f16")
        else:
            h = check_ptr(ffi.lib().mse_scores_from_base(self._h, vecs._h, ip, first, count, tp), "mse_scores_from_base")
        return RowScores(h)

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_score_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _timestamps(timestamps, count):
    """(int64 array or None, pointer or None); the array must outlive the call."""
    if timestamps is None:
        return None, None
    t = np.asarray(timestamps)
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise TypeError("timestamps must be integers")
    if t.size and t.dtype == np.uint64 and t.max() > 0x7FFFFFFFFFFFFFFF:
        raise MseError("a timestamp is outside [0, 2**32)")
    t = np.ascontiguousarray(t.reshape(-1), np.int64)
    if t.size != count:
        raise ValueError(f"timestamps must hold one entry per row: {t.size} for {count} rows")
    return t, _p(t, C.c_int64)


class RowScores:
    """A device-resident score table (mse_scores): [n, channels] float32, plus a uint32 timestamp channel when one was given -- channel
    index `channels`, the last descriptor.  n_desc = channels (+ 1)."""

    def __init__(self, handle):
        self._h = handle
        self.channels = int(ffi.lib().mse_scores_channels(handle))
        self.has_timestamps = bool(ffi.lib().mse_scores_has_timestamps(handle))
        self.n_desc = self.channels + (1 if self.has_timestamps else 0)

    @classmethod
    def from_host(cls, scores, timestamps=None):
        s = np.ascontiguousarray(scores, np.float32)
        if s.ndim != 2:
            raise MseError("scores must be [n, channels]")
        ts, tp = _timestamps(timestamps, s.shape[0])
        return cls(check_ptr(ffi.lib().mse_scores_from_host(_p(s, C.c_float), s.shape[0], s.shape[1], tp), "mse_scores_from_host"))

    def __len__(self):
        return int(ffi.lib().mse_scores_len(self._h))

    def to_host(self):
        """scores float32 [n, channels]; with timestamps: (scores, timestamps uint32 [n])."""
        out = np.empty((len(self), self.channels), np.float32)
        ts = np.empty(len(self), np.uint32) if self.has_timestamps else None
        check(ffi.lib().mse_scores_read(self._h, _p(out, C.c_float), _p(ts, C.c_uint32) if ts is not None else None), "scores_read")
        return (out, ts) if self.has_timestamps else out

    def order_statistics(self, channel, ranks):
        """numpy.sort(column)[ranks] without sorting (mse_scores_order_statistics), exact: float32 for a score channel (+-0 are one key),
        uint32 for the timestamp channel (index `channels`).  A NaN among the keys is an error that counts them."""
        r = np.asarray(ranks)
        if r.size and (not np.issubdtype(r.dtype, np.integer) or r.min() < 0):
            raise ValueError("ranks must be non-negative integers")
        r = np.ascontiguousarray(r.reshape(-1), np.uint64)
        out = np.empty(r.size, np.float64)
        check(ffi.lib().mse_scores_order_statistics(self._h, int(channel), _p(r, C.c_uint64), r.size, _p(out, C.c_double)), "order_statistics")
        return out.astype(np.uint32 if int(channel) == self.channels else np.float32)

    def fit_cdfs(self, cdf_len=255):
        """float32 [n_desc, cdf_len]: numpy.quantile(channel, numpy.linspace(0, 1, cdf_len)) of every channel, the timestamps last
        (meme-rater/compute_cdf.py:64-71) -- IndexHeader.descriptor_cdfs as it stands."""
        out = np.empty((self.n_desc, int(cdf_len)), np.float32)
        check(ffi.lib().mse_scores_fit_cdfs(self._h, int(cdf_len), _p(out, C.c_float)), "fit_cdfs")
        return out

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_scores_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def descriptor_buckets(cdfs, scores):
    """dump_processor.rs:483-491: scores [n, n_desc] -> bytes [n, n_desc] through the ascending CDF of each channel."""
    c = np.ascontiguousarray(cdfs, np.float32)
    s = np.ascontiguousarray(scores, np.float32)
    if c.ndim != 2 or s.ndim != 2 or s.shape[1] != c.shape[0]:
        raise MseError("cdfs must be [n_desc, cdf_len] and scores [n, n_desc]")
    out = np.empty(s.shape, np.uint8)
    check(ffi.lib().mse_descriptor_buckets(_p(c, C.c_float), c.shape[0], c.shape[1], _p(s, C.c_float), s.shape[0], _p(out, C.c_uint8)),
          "descriptor_buckets")
    return out
