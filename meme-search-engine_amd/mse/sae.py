"""Sparse-autoencoder features of a resident index: the reference's sae/ (model.py, export_features.py, train.py) on the device.
SparseAutoencoder holds a checkpoint trained by sae/train.py or by SaeTrainer below; encode_rows turns resident f16 rows into RowFeatures -- per row at most
top_k (feature, activation) pairs, on the device -- from which come the feature counters (model.py:23-29,42), the reconstruction and its
squared error (train.py:55-56), and a RowFilter per feature.  The arithmetic is fixed (csrc/sae.hip); tests/sae_ref.py restates it.
SaeTrainer is train.py:51-59 -- mse_loss, backward, AdamW -- over the same resident rows, updating the model's device weights in place
(csrc/sae_train.hip; tests/sae_train_ref.py restates it)."""
import ctypes as C

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr
from .vector import RowFilter, _bits, _p

NONE = 0xFFFFFFFF   # an unused feature slot; the count of an invalid row


def _f32(a, shape_name, ndim):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float32)
    if a.ndim != ndim:
        raise MseError(f"sparse autoencoder: {shape_name} must have {ndim} dimension(s)")
    return a


class SparseAutoencoder:
    """sae/model.py:16-43.  up [d_hidden, d_emb] (up_proj.weight), down [d_emb, d_hidden] (down_proj.weight), optional up_bias [d_hidden]
    and down_bias [d_emb]; numpy arrays or torch tensors, float32.  1 <= top_k <= 256, top_k < d_hidden."""

    def __init__(self, up, down, up_bias=None, down_bias=None, top_k=128):
        up, down = _f32(up, "up", 2), _f32(down, "down", 2)
        ub = None if up_bias is None else _f32(up_bias, "up_bias", 1)
        db = None if down_bias is None else _f32(down_bias, "down_bias", 1)
        if down.shape != up.shape[::-1] or (ub is not None and ub.size != up.shape[0]) or (db is not None and db.size != up.shape[1]):
            raise MseError("sparse autoencoder: inconsistent tensor shapes")
        self.d_hidden, self.d_emb, self.top_k = up.shape[0], up.shape[1], int(top_k)
        self._down, self._down_stale = down, False   # kept on the host for feature_queries; stale after a training call
        self.has_up_bias, self.has_down_bias = ub is not None, db is not None
        self._h = check_ptr(ffi.lib().mse_sae_load(_p(up, C.c_float), None if ub is None else _p(ub, C.c_float), _p(down, C.c_float),
                                                   None if db is None else _p(db, C.c_float), self.d_emb, self.d_hidden, self.top_k), "mse_sae_load")

    @classmethod
    def random(cls, d_emb, d_hidden, top_k, seed, up_proj_bias=False):
        """The initialisation of sae/model.py:20-22 from numpy's default_rng(seed): up ~ U(+-1/sqrt(d_emb)) (nn.Linear's default),
        down = up transposed, down_bias ~ U(+-1/sqrt(d_hidden)), up_bias ~ U(+-1/sqrt(d_emb)) with up_proj_bias.  torch's
        distribution, not torch's bits."""
        rng = np.random.default_rng(seed)
        bu, bd = 1.0 / np.sqrt(d_emb), 1.0 / np.sqrt(d_hidden)
        up = rng.uniform(-bu, bu, (d_hidden, d_emb)).astype(np.float32)
        ub = rng.uniform(-bu, bu, d_hidden).astype(np.float32) if up_proj_bias else None
        db = rng.uniform(-bd, bd, d_emb).astype(np.float32)
        return cls(up, np.ascontiguousarray(up.T), ub, db, top_k=top_k)

    @property
    def down(self):
        """down_proj.weight [d_emb, d_hidden] on the host (re-read after a training call)"""
        if self._down_stale:
            self._down, self._down_stale = self.weights()[1], False
        return self._down

    def weights(self):
        """(up [d_hidden, d_emb], down [d_emb, d_hidden], up_bias or None, down_bias or None): the current device weights, float32 --
        the arguments of SparseAutoencoder(...)."""
        up, down = np.empty((self.d_hidden, self.d_emb), np.float32), np.empty((self.d_emb, self.d_hidden), np.float32)
        ub = np.empty(self.d_hidden, np.float32) if self.has_up_bias else None
        db = np.empty(self.d_emb, np.float32) if self.has_down_bias else None
        check(ffi.lib().mse_sae_read_weights(self._h, _p(up, C.c_float), None if ub is None else _p(ub, C.c_float), _p(down, C.c_float),
                                             None if db is None else _p(db, C.c_float)), "sae_read_weights")
        return up, down, ub, db

    @classmethod
    def from_state_dict(cls, sd, top_k):
        """The "model" entry of a checkpoint saved by sae/train.py:65-69: up_proj.weight, down_proj.weight, down_proj.bias and -- with
        up_proj_bias -- up_proj.bias."""
        up, down, ub, db = cls.state_dict_tensors(sd)
        return cls(up, down, ub, db, top_k=top_k)

    @staticmethod
    def state_dict_tensors(sd):
        """(up [d_hidden, d_emb], down [d_emb, d_hidden], up_bias or None, down_bias or None) of a state dict, as float32 numpy arrays"""
        ub, db = sd.get("up_proj.bias"), sd.get("down_proj.bias")
        return (_f32(sd["up_proj.weight"], "up_proj.weight", 2), _f32(sd["down_proj.weight"], "down_proj.weight", 2),
                None if ub is None else _f32(ub, "up_proj.bias", 1), None if db is None else _f32(db, "down_proj.bias", 1))

    def set_hidden_parts(self, parts):
        """Test and probe hook: workgroups that share d_hidden per row tile; 0 = automatic.  The features do not depend on it."""
        check(ffi.lib().mse_sae_set_hidden_parts(self._h, int(parts)), "sae_set_hidden_parts")

    def encode_rows(self, vecs_or_searcher, ids=None, first=0, n=None, count=True):
        """SAE.forward up to the mask (model.py:31-41) over rows resident in HBM (mse_sae_encode_base): rows `ids` (any order, repeats
        allowed) or first .. first + n (n None: to the end) of a VectorList or of a Searcher's rows.  A 2-D numpy array of f16 rows
        (np.float16 or uint16 bits, any width) is uploaded -- the selected rows of it -- and encoded by the same kernels
        (mse_sae_encode_f16).  count: add the kept features to the counters.  A row's features are the same bits however it is asked
        for.  Returns a RowFeatures (on the device); one over a VectorList borrows its rows."""
        sel = None
        if ids is not None:
            i = np.asarray(ids)
            if i.size and not np.issubdtype(i.dtype, np.integer):
                raise TypeError("ids must be an integer array")
            i = i.reshape(-1)
            if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
                raise ValueError("ids must be in 0 .. 2**32 - 1")
            sel = np.ascontiguousarray(i, np.uint32)
        if isinstance(vecs_or_searcher, np.ndarray):
            host = _bits(vecs_or_searcher)
            if host.ndim != 2:
                raise MseError("encode_rows: host rows must be [n_rows, d]")
            if sel is not None:
                if sel.size and sel.max() >= host.shape[0]:
                    raise MseError(f"encode_rows: id {int(sel.max())} is not below the {host.shape[0]} rows")
                host = host[sel.astype(np.int64)]
            else:
                first = int(first)
                count_rows = host.shape[0] - first if n is None else int(n)
                if first < 0 or count_rows < 0 or first + count_rows > host.shape[0]:
                    raise ValueError("row range out of bounds")
                host = host[first:first + count_rows]
            return self.encode(host, count=count)
        vecs = getattr(vecs_or_searcher, "vecs", vecs_or_searcher)
        if getattr(vecs, "_h", None) is None:
            raise MseError("encode_rows needs a VectorList, a Searcher over one, or a 2-D array of f16 rows")
        if sel is not None:
            ip, cnt, first = _p(sel, C.c_uint32), sel.size, 0
        else:
            first = int(first)
            cnt = len(vecs) - first if n is None else int(n)
            if first < 0 or cnt < 0:
                raise ValueError("row range out of bounds")
            ip = None
        h = check_ptr(ffi.lib().mse_sae_encode_base(self._h, vecs._h, ip, first, cnt, int(bool(count))), "mse_sae_encode_base")
        return RowFeatures(h, self, keep=vecs)

    def encode(self, rows_f16, count=True):
        """encode_rows over f16 rows on the host, [n, d_emb]; the table keeps a device copy of them and its filters speak of rows 0 .. n."""
        host = np.ascontiguousarray(_bits(rows_f16))
        if host.ndim != 2:
            raise MseError("encode: host rows must be [n_rows, d]")
        h = check_ptr(ffi.lib().mse_sae_encode_f16(self._h, _p(host, C.c_uint16), host.shape[0], host.shape[1], int(bool(count))), "mse_sae_encode_f16")
        return RowFeatures(h, self)

    def counters(self, reset=False):
        """feature_activation_counter (model.py:23,42) as uint64 [d_hidden]; reset=True is reset_counters (model.py:26-29): the old values
        come back and the counters are zeroed."""
        out = np.empty(self.d_hidden, np.uint64)
        check(ffi.lib().mse_sae_counters(self._h, _p(out, C.c_uint64), int(bool(reset))), "sae_counters")
        return out

    def feature_queries(self, features, sign=1):
        """The decoder columns of `features` narrowed to f16, [len(features), d_emb] uint16 bits, ready for Searcher.bruteforce_topk: the
        exemplar queries of sae/export_features.py:56-57,80-81 (sign=-1: the negative exemplars)."""
        f = np.asarray(features, np.int64).reshape(-1)
        if f.size and (f.min() < 0 or f.max() >= self.d_hidden):
            raise ValueError("features must be in 0 .. d_hidden - 1")
        cols = self.down[:, f].T * np.float32(1 if sign >= 0 else -1)
        return np.ascontiguousarray(cols.astype(np.float16)).view(np.uint16)

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_sae_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowFeatures:
    """A device-resident feature table (mse_features): per row a count, and top_k (feature, activation) slots in canonical order --
    activation descending, feature ascending; unused slots hold feature 0xFFFFFFFF and activation +0.  An invalid row (a NaN
    pre-activation) has count 0xFFFFFFFF and no features."""

    def __init__(self, handle, model, keep=None):
        self._h, self._model, self._keep = handle, model, keep
        self.top_k = int(ffi.lib().mse_features_top_k(handle))
        self.invalid_rows = int(ffi.lib().mse_features_invalid_rows(handle))
        self._host = None

    def __len__(self):
        return int(ffi.lib().mse_features_len(self._h))

    def to_host(self):
        """(counts uint32 [n], features uint32 [n, top_k], activations float32 [n, top_k])"""
        if self._host is None:
            n = len(self)
            c, f, a = np.empty(n, np.uint32), np.empty((n, self.top_k), np.uint32), np.empty((n, self.top_k), np.float32)
            check(ffi.lib().mse_features_read(self._h, _p(c, C.c_uint32), _p(f, C.c_uint32), _p(a, C.c_float)), "features_read")
            self._host = (c, f, a)
        return self._host

    counts = property(lambda self: self.to_host()[0])
    features = property(lambda self: self.to_host()[1])
    activations = property(lambda self: self.to_host()[2])

    def _recon(self, want_recon, want_sq, model=None):
        m = self._model if model is None else model
        n = len(self)
        r = np.empty((n, m.d_emb), np.float32) if want_recon else None
        s = np.empty(n, np.float64) if want_sq else None
        check(ffi.lib().mse_features_reconstruct(self._h, m._h, None if r is None else _p(r, C.c_float), None if s is None else _p(s, C.c_double)),
              "features_reconstruct")
        return r, s

    def reconstruct(self, model=None):
        """down_proj over the kept features (model.py:43), float32 [n, d_emb]; NaN for an invalid row."""
        return self._recon(True, False, model)[0]

    def sq_errors(self, model=None):
        """Per row the squared error of the reconstruction against the row, float64 [n]; NaN for an invalid row."""
        return self._recon(False, True, model)[1]

    def mse(self, model=None):
        """F.mse_loss(reconstructions, batch) of sae/train.py:56 over the valid rows: the mean over rows x d_emb."""
        s = self.sq_errors(model)
        ok = ~np.isnan(s)
        m = self._model if model is None else model
        return float(s[ok].sum() / (ok.sum() * m.d_emb)) if ok.any() else float("nan")

    def filter(self, feature, min_activation=0.0, n_rows=None):
        """The rows that keep `feature` with an activation >= min_activation as a RowFilter over base row ids (mse_features_filter);
        n_rows: the filter's length (default: the base's rows; the table's rows for one made from host rows)."""
        if n_rows is None:
            n_rows = len(self._keep) if self._keep is not None else len(self)
        return RowFilter.from_handle(check_ptr(ffi.lib().mse_features_filter(self._h, int(feature), float(min_activation), int(n_rows)),
                                               "mse_features_filter"))

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_features_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StepRefused(MseError):
    """A training step met an invalid (NaN) row or a non-finite loss and changed nothing; .steps_done steps of the call completed
    before it and .losses holds their losses."""

    def __init__(self, steps_done, losses):
        super().__init__(f"sparse-autoencoder training: step {steps_done} of the call was refused (a NaN row or a non-finite loss); "
                         f"{steps_done} step(s) completed")
        self.steps_done, self.losses = steps_done, losses


class SaeTrainer:
    """sae/train.py:51-59 over a SparseAutoencoder: F.mse_loss, backward and torch.optim.AdamW (decoupled decay), on the device, in
    place on the model's weights.  The model needs a down_bias.  The arithmetic is fixed, so a run is the same bytes however it is cut
    into calls."""

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.model = model
        self._h = check_ptr(ffi.lib().mse_sae_trainer_create(model._h, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)),
                            "mse_sae_trainer_create")

    @property
    def steps(self):
        """completed steps (torch's `step`)"""
        return int(ffi.lib().mse_sae_trainer_step_count(self._h))

    def train(self, source, ids, batch_size):
        """One step per batch_size consecutive entries of ids (rows of `source`: whatever encode_rows takes -- a VectorList, a Searcher
        over one, or a 2-D array of f16 rows); a ragged last batch is dropped (train.py:88).  The ids are uploaded once and the steps
        queued without a host round trip.  Returns the losses, float64 [steps]; raises StepRefused where a step was refused."""
        i = np.asarray(ids)
        if i.size and not np.issubdtype(i.dtype, np.integer):
            raise TypeError("ids must be an integer array")
        i = i.reshape(-1)
        if i.size and (i.min() < 0 or i.max() > 0xFFFFFFFF):
            raise ValueError("ids must be in 0 .. 2**32 - 1")
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        n_steps = i.size // batch_size
        sel = np.ascontiguousarray(i[:n_steps * batch_size], np.uint32)
        losses, done = np.zeros(n_steps, np.float64), C.c_size_t(0)
        lp = _p(losses, C.c_double)
        self.model._down_stale = True
        if isinstance(source, np.ndarray):
            host = _bits(source)
            if host.ndim != 2:
                raise MseError("train: host rows must be [n_rows, d]")
            if sel.size and sel.max() >= host.shape[0]:
                raise MseError(f"train: id {int(sel.max())} is not below the {host.shape[0]} rows")
            rows = np.ascontiguousarray(host[sel.astype(np.int64)])
            check(ffi.lib().mse_sae_trainer_steps_f16(self._h, _p(rows, C.c_uint16), host.shape[1], batch_size, n_steps, lp, C.byref(done)),
                  "sae_trainer_steps_f16")
        else:
            vecs = getattr(source, "vecs", source)
            if getattr(vecs, "_h", None) is None:
                raise MseError("train needs a VectorList, a Searcher over one, or a 2-D array of f16 rows")
            check(ffi.lib().mse_sae_trainer_steps(self._h, vecs._h, _p(sel, C.c_uint32), batch_size, n_steps, lp, C.byref(done)), "sae_trainer_steps")
        if done.value < n_steps:
            raise StepRefused(int(done.value), losses[:done.value].copy())
        return losses

    def step(self, source, ids):
        """One step over the rows `ids` of source; returns its loss (before the update)."""
        n = int(np.asarray(ids).size)
        if n < 1:
            raise ValueError("an empty batch")
        return float(self.train(source, ids, n)[0])

    def set_skip(self, on):
        """Test and probe hook: whether the dense update may leave out never-touched feature rows (weight_decay = 0).  Same bytes."""
        check(ffi.lib().mse_sae_trainer_set_skip(self._h, int(bool(on))), "sae_trainer_set_skip")

    _STATE = ("m_up", "v_up", "m_up_bias", "v_up_bias", "m_down", "v_down", "m_down_bias", "v_down_bias")

    def state(self):
        """{"t": steps, "m_*" / "v_*": exp_avg / exp_avg_sq of up [d_hidden, d_emb], up_bias (with one), down [d_emb, d_hidden],
        down_bias}: numpy arrays, the checkpoint's layout."""
        m = self.model
        shapes = {"up": (m.d_hidden, m.d_emb), "up_bias": (m.d_hidden,), "down": (m.d_emb, m.d_hidden), "down_bias": (m.d_emb,)}
        out = {k: np.zeros(shapes[k[2:]], np.float32) for k in self._STATE if m.has_up_bias or "up_bias" not in k}
        t = C.c_uint64(0)
        check(ffi.lib().mse_sae_trainer_state_read(self._h, C.byref(t), *[None if k not in out else _p(out[k], C.c_float) for k in self._STATE]),
              "sae_trainer_state_read")
        out["t"] = int(t.value)
        return out

    def load_state(self, state):
        m = self.model
        shapes = {"up": (m.d_hidden, m.d_emb), "up_bias": (m.d_hidden,), "down": (m.d_emb, m.d_hidden), "down_bias": (m.d_emb,)}
        args = []
        for k in self._STATE:
            if "up_bias" in k and not m.has_up_bias:
                args.append(None)
                continue
            a = np.ascontiguousarray(state[k], np.float32)
            if a.shape != shapes[k[2:]]:
                raise MseError(f"load_state: {k} has shape {a.shape}, not {shapes[k[2:]]}")
            args.append(a)
        check(ffi.lib().mse_sae_trainer_state_write(self._h, int(state["t"]), *[None if a is None else _p(a, C.c_float) for a in args]),
              "sae_trainer_state_write")

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_sae_trainer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
