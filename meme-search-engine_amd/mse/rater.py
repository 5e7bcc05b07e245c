"""The ensemble rater of the reference's meme-rater/ on the device: the quality model whose scores become the descriptor bytes.
Rater holds n_members one-hidden-layer MLPs (model.py:18-38) in the wide layout of ensemble_to_wide_model.py:44-55; RaterTrainer is
train.py:63-71 -- binary cross-entropy on the Bradley-Terry win probabilities, backward, AdamW -- over rated pairs of resident rows,
in place on the device weights; MemberScores is every member's score of resident rows, over which pair_variance / top_pairs rank
candidate pairs by the members' disagreement (active_learning.py:44-60); Rater.to_score_model is the export the descriptor path takes.
The arithmetic is fixed (csrc/rater.hip, csrc/rater_math.h); tests/rater_ref.py restates it."""
import ctypes as C
import math

import numpy as np

from . import ffi
from .ffi import MseError, check, check_ptr
from .sae import StepRefused
from .vector import _bits, _p

_RATINGS = {"1": 0.9, "2": 0.1, "2+": 0.3, "2p": 0.3, "1+": 0.7, "1p": 0.7, "eq": 0.5}


def map_rating(rating):
    """shared.py:23-38: "1,2+,eq" -> the target win probability of the first meme per channel, float64 [channels]"""
    out = []
    for r in rating.split(","):
        if r not in _RATINGS:
            raise ValueError("invalid rating, please fix")
        out.append(_RATINGS[r])
    return np.array(out)


def _f32(a, name, ndim):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float32)
    if a.ndim != ndim:
        raise MseError(f"rater: {name} must have {ndim} dimension(s)")
    return a


def _u32(a, name):
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must be an integer array")
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError(f"{name} must be in 0 .. 2**32 - 1")
    return np.ascontiguousarray(a, np.uint32)


def _source(source, who):
    """(host f16 bits [n, d] or None, VectorList or None)"""
    if isinstance(source, np.ndarray):
        host = np.ascontiguousarray(_bits(source))
        if host.ndim != 2:
            raise MseError(f"{who}: host rows must be [n_rows, d]")
        return host, None
    vecs = getattr(source, "vecs", source)
    if getattr(vecs, "_h", None) is None:
        raise MseError(f"{who} needs a VectorList, a Searcher over one, or a 2-D array of f16 rows")
    return None, vecs


class RaterStepRefused(StepRefused):
    """StepRefused as the rater's trainer raises it: a training step met a non-finite row or a non-finite loss and changed nothing;
    .steps_done steps of the call completed before it and .losses holds their losses."""

    def __init__(self, steps_done, losses):
        MseError.__init__(self, f"rater training: step {steps_done} of the call was refused (a non-finite row or a non-finite loss); "
                                f"{steps_done} step(s) completed")
        self.steps_done, self.losses = steps_done, losses


class Rater:
    """model.py:31-38 in the wide layout: up [n_members * d_emb, d_emb], bias [n_members * d_emb], down [out_channels, n_members *
    d_emb]; numpy arrays or torch tensors, float32.  Member m owns hidden units m * d_emb .. (m + 1) * d_emb."""

    def __init__(self, up, bias, down, n_members):
        up, bias, down = _f32(up, "up", 2), _f32(bias, "bias", 1), _f32(down, "down", 2)
        M = int(n_members)
        if M < 1 or up.shape[0] != M * up.shape[1] or bias.size != up.shape[0] or down.shape[1] != up.shape[0]:
            raise MseError("rater: inconsistent tensor shapes")
        self.d_emb, self.n_members, self.out_channels = up.shape[1], M, down.shape[0]
        self._h = check_ptr(ffi.lib().mse_rater_create(_p(up, C.c_float), _p(bias, C.c_float), _p(down, C.c_float), self.d_emb, M,
                                                       self.out_channels), "mse_rater_create")

    @classmethod
    def from_wide(cls, up, bias, down, n_members):
        """The tensors of a model.safetensors written by ensemble_to_wide_model.py:76-80 (up_proj, bias, down_proj) and its member count"""
        return cls(up, bias, down, n_members)

    @classmethod
    def random(cls, d_emb, n_members, out_channels, rng, dropout=0.0):
        """A fresh ensemble (model.py:21-23): both layers of every member from nn.Linear's default U(+-1/sqrt(d_emb)), drawn from the numpy
        Generator `rng` -- torch's distribution, not torch's bits.  The output bias is not carried."""
        if dropout != 0.0:
            raise MseError("rater: dropout other than 0 is not supported (train.py:40 trains with 0.0 and evaluation disables it)")
        b = 1.0 / math.sqrt(d_emb)
        H = n_members * d_emb
        up = rng.uniform(-b, b, (H, d_emb)).astype(np.float32)
        bias = rng.uniform(-b, b, H).astype(np.float32)
        down = rng.uniform(-b, b, (out_channels, H)).astype(np.float32)
        return cls(up, bias, down, n_members)

    def weights(self):
        """(up, bias, down): the current device weights in the wide layout, float32 -- the arguments of from_wide"""
        H = self.n_members * self.d_emb
        up, bias, down = np.empty((H, self.d_emb), np.float32), np.empty(H, np.float32), np.empty((self.out_channels, H), np.float32)
        check(ffi.lib().mse_rater_read_weights(self._h, _p(up, C.c_float), _p(bias, C.c_float), _p(down, C.c_float)), "rater_read_weights")
        return up, bias, down

    def to_score_model(self):
        """ensemble_to_wide_model.py:76-80: the wide ScoreModel of the current weights; its d_emb / d_hidden scale is 1 / n_members, so its
        score is the mean over the members.  Through the host: a ScoreModel takes host arrays."""
        from .index_pack import ScoreModel
        return ScoreModel(*self.weights())

    def member_scores(self, source, ids=None, first=0, n=None):
        """Every member's scores of rows resident in HBM: rows `ids` (any order, repeats allowed) or first .. first + n (n None: to the
        end) of a VectorList, of a Searcher's rows, or of a 2-D numpy array of f16 rows (uploaded for the call).  A row's scores are the
        same bits however it is asked for.  Returns a MemberScores (on the device)."""
        host, vecs = _source(source, "member_scores")
        n_rows = host.shape[0] if host is not None else len(vecs)
        if ids is not None:
            sel = _u32(np.asarray(ids).reshape(-1), "ids")
            ip, cnt, first = _p(sel, C.c_uint32), sel.size, 0
        else:
            first = int(first)
            cnt = n_rows - first if n is None else int(n)
            if first < 0 or cnt < 0:
                raise ValueError("row range out of bounds")
            ip = None
        if host is not None:
            h = check_ptr(ffi.lib().mse_member_scores_from_f16(self._h, _p(host, C.c_uint16), host.shape[0], host.shape[1], ip, first, cnt),
                          "mse_member_scores_from_f16")
        else:
            h = check_ptr(ffi.lib().mse_member_scores_from_base(self._h, vecs._h, ip, first, cnt), "mse_member_scores_from_base")
        return MemberScores(h, self.n_members, self.out_channels)

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_rater_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MemberScores:
    """A device-resident table [n, n_members, out_channels] of member scores (mse_member_scores): model.py:38's stacked outputs, without
    the output bias."""

    def __init__(self, handle, n_members, out_channels):
        self._h, self.n_members, self.out_channels = handle, n_members, out_channels

    def __len__(self):
        return int(ffi.lib().mse_member_scores_len(self._h))

    def to_host(self):
        out = np.empty((len(self), self.n_members, self.out_channels), np.float32)
        check(ffi.lib().mse_member_scores_read(self._h, _p(out, C.c_float)), "member_scores_read")
        return out

    def pair_variance(self, a, b):
        """active_learning.py:50-53 for the pairs (a[i], b[i]) of table rows: the variance over the members (torch.var's default
        correction) of the win probabilities, the largest over the channels; float32 [n_pairs]."""
        a, b = _u32(np.asarray(a).reshape(-1), "a"), _u32(np.asarray(b).reshape(-1), "b")
        if a.size != b.size:
            raise MseError("pair_variance: a and b differ in length")
        out = np.empty(a.size, np.float32)
        check(ffi.lib().mse_member_scores_pair_variance(self._h, _p(a, C.c_uint32), _p(b, C.c_uint32), a.size, _p(out, C.c_float)),
              "member_scores_pair_variance")
        return out

    def top_pairs(self, a, b, k):
        """active_learning.py:58-60: (indices into a / b, variances) of the k pairs the members disagree on most -- variance descending,
        pair index ascending.  The order is made on the host from pair_variance's floats."""
        var = self.pair_variance(a, b)
        order = np.lexsort((np.arange(var.size), -var.astype(np.float64)))[:int(k)]
        return order, var[order]

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_member_scores_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RaterTrainer:
    """train.py:56-71 over a Rater: F.binary_cross_entropy on the win probabilities, backward and torch.optim.AdamW (decoupled decay), on
    the device, in place on the rater's weights.  The arithmetic is fixed, so a run is the same bytes however it is cut into calls."""

    def __init__(self, rater, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dropout=0.0):
        if dropout != 0.0:
            raise MseError("rater: dropout other than 0 is not supported (train.py:40 trains with 0.0 and evaluation disables it)")
        self.rater = rater
        self._h = check_ptr(ffi.lib().mse_rater_trainer_create(rater._h, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)),
                            "mse_rater_trainer_create")

    @property
    def steps(self):
        """completed steps (torch's `step`)"""
        return int(ffi.lib().mse_rater_trainer_step_count(self._h))

    def run(self, source, pair_ids, targets):
        """One step per leading entry: pair_ids [n_steps, n_members, batch, 2] rows of `source` (a VectorList, a Searcher over one, or a
        2-D array of f16 rows) -- each member its own pairs -- and targets [n_steps, n_members, batch, out_channels] in [0, 1].  The ids
        are uploaded once and the steps queued without a host round trip.  Returns the losses, float64 [n_steps]; raises StepRefused
        where a step was refused."""
        r = self.rater
        ids = _u32(pair_ids, "pair_ids")
        y = np.ascontiguousarray(targets, np.float32)
        if ids.ndim != 4 or ids.shape[1] != r.n_members or ids.shape[3] != 2:
            raise MseError(f"run: pair_ids must be [n_steps, {r.n_members}, batch, 2]")
        n_steps, _, batch, _ = ids.shape
        if y.shape != (n_steps, r.n_members, batch, r.out_channels):
            raise MseError(f"run: targets must be {(n_steps, r.n_members, batch, r.out_channels)}, not {y.shape}")
        losses, done = np.zeros(n_steps, np.float64), C.c_size_t(0)
        host, vecs = _source(source, "run")
        if host is not None:
            check(ffi.lib().mse_rater_trainer_steps_f16(self._h, _p(host, C.c_uint16), host.shape[0], host.shape[1], _p(ids, C.c_uint32), _p(y, C.c_float),
                                                        batch, n_steps, _p(losses, C.c_double), C.byref(done)), "rater_trainer_steps_f16")
        else:
            check(ffi.lib().mse_rater_trainer_steps(self._h, vecs._h, _p(ids, C.c_uint32), _p(y, C.c_float), batch, n_steps, _p(losses, C.c_double),
                                                    C.byref(done)), "rater_trainer_steps")
        if done.value < n_steps:
            raise RaterStepRefused(int(done.value), losses[:done.value].copy())
        return losses

    def train(self, source, pairs, ratings, epochs, rng, batch_size=1):
        """train.py:114-119: per epoch one permutation of the rated pairs per member (shared.generate_random_permutations) from the numpy
        Generator `rng`, cut into batches of batch_size; a ragged last batch runs as a shorter step of its own (:117-118 slices and does
        not drop).  pairs [n, 2] rows of source, ratings [n, out_channels] targets (map_rating).  Returns the losses of every step."""
        pairs = _u32(pairs, "pairs")
        y = np.ascontiguousarray(ratings, np.float32)
        M = self.rater.n_members
        if pairs.ndim != 2 or pairs.shape[1] != 2 or y.shape != (pairs.shape[0], self.rater.out_channels):
            raise MseError("train: pairs must be [n, 2] and ratings [n, out_channels]")
        n, batch_size = pairs.shape[0], int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        losses = []
        for _ in range(int(epochs)):
            orders = np.stack([rng.permutation(n) for _ in range(M)])      # [M, n]
            whole = n // batch_size
            if whole:
                o = orders[:, :whole * batch_size].reshape(M, whole, batch_size).transpose(1, 0, 2)
                losses.append(self.run(source, pairs[o], y[o]))
            if n % batch_size:
                o = orders[:, whole * batch_size:][None]
                losses.append(self.run(source, pairs[o], y[o]))
        return np.concatenate(losses) if losses else np.zeros(0, np.float64)

    def last_scores(self):
        """test hook: the forward pass's scores [n_members, 2 * batch, out_channels] of the last completed step of the last call"""
        b = C.c_size_t(0)
        check(ffi.lib().mse_rater_trainer_last_scores(self._h, None, C.byref(b)), "rater_trainer_last_scores")
        out = np.empty((self.rater.n_members, 2 * b.value, self.rater.out_channels), np.float32)
        check(ffi.lib().mse_rater_trainer_last_scores(self._h, _p(out, C.c_float), None), "rater_trainer_last_scores")
        return out

    _STATE = ("m_up", "v_up", "m_bias", "v_bias", "m_down", "v_down")

    def _shapes(self):
        r = self.rater
        H = r.n_members * r.d_emb
        return {"up": (H, r.d_emb), "bias": (H,), "down": (r.out_channels, H)}

    def state(self):
        """{"t": steps, "m_*" / "v_*": exp_avg / exp_avg_sq of up, bias and down}: numpy arrays in the wide layout"""
        shapes = self._shapes()
        out = {k: np.zeros(shapes[k[2:]], np.float32) for k in self._STATE}
        t = C.c_uint64(0)
        check(ffi.lib().mse_rater_trainer_state_read(self._h, C.byref(t), *[_p(out[k], C.c_float) for k in self._STATE]), "rater_trainer_state_read")
        out["t"] = int(t.value)
        return out

    def load_state(self, state):
        shapes = self._shapes()
        args = []
        for k in self._STATE:
            a = np.ascontiguousarray(state[k], np.float32)
            if a.shape != shapes[k[2:]]:
                raise MseError(f"load_state: {k} has shape {a.shape}, not {shapes[k[2:]]}")
            args.append(a)
        check(ffi.lib().mse_rater_trainer_state_write(self._h, int(state["t"]), *[_p(a, C.c_float) for a in args]), "rater_trainer_state_write")

    def close(self):
        if getattr(self, "_h", None):
            ffi.lib().mse_rater_trainer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
