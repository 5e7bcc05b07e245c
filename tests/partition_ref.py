"""Numpy restatement of the shard partition (include/mse.h mse_partitioner), shared by tests/test_partition_host.py and
tests/test_gpu_partition.py.  Everything is stated in IEEE double / single operations that numpy performs one at a time, in the order the
header gives, so the device has to reproduce the bits: the score is a k-ascending float64 chain (float64 products of an f16 and an f32 value
are exact), sums of squares and the Newton square root run in Python floats, the temperature in np.float32."""
import numpy as np

K = np.float32(np.float64(1.7320508075688772) / 65536.0)     # (float)(sqrt(3) / 65536)
DEFAULTS = dict(temperature0=1.0, accept_decay=0.999, reject_decay=0.9995, reroll_heat=1.1, temperature_cap=1.5, reroll_after=100, seed=0,
                stop_fraction=0.1)


def widen(x16):
    return np.asarray(x16, np.uint16).view(np.float16).astype(np.float32)


def skewed_rows(orc, n, seed_base, seed_centres, d=1152):
    """x = f16(normalise(gen_rows(seed_base) + 0.75 P[lab])), P = 3 rows of gen_rows(seed_centres), lab = min(i % 10, 5) // 2: three
    clusters of 40 %, 40 % and 20 % of the rows, so random centroids start far from balance."""
    x = widen(orc.gen_rows_f16(seed_base, 0, n, d)).astype(np.float64)
    P = widen(orc.gen_rows_f16(seed_centres, 0, 3, d)).astype(np.float64)
    lab = np.minimum(np.arange(n) % 10, 5) // 2
    x = x + 0.75 * P[lab]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float16).view(np.uint16))


def noise(orc, seed, key, d):
    return orc.gen_row_ints(seed, key, d).astype(np.float32) * K


def normalise(c):
    c = np.asarray(c, np.float32)
    out = np.empty_like(c)
    for s in range(c.shape[0]):
        row = c[s].astype(np.float64)
        ss = 0.0
        for x in row.tolist():
            ss = ss + x * x
        if ss > 0.0:
            y = 1.0
            for _ in range(48):
                y = 0.5 * (y + ss / y)
            out[s] = (row / y).astype(np.float32)
        else:
            out[s] = c[s]
    return out


def scores(x16, c):
    """[n][S] float64: acc = acc + x_k c_k for k ascending, every operation one IEEE double operation"""
    x = widen(x16).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float64)
    for k in range(x.shape[1]):
        acc = acc + x[:, k, None] * c[None, :, k]
    return acc


def top2(sc):
    """(best, second) per row: score descending, lowest index on ties (np.argmax returns the first maximum)"""
    i1 = np.argmax(sc, axis=1)
    rest = sc.copy()
    rest[np.arange(sc.shape[0]), i1] = -np.inf
    i2 = np.argmax(rest, axis=1)
    same = i2 == i1                                   # only when every other score is -inf: not reached by finite rows
    i2[same] = np.where(i1[same] == 0, 1, 0)
    return np.stack([i1, i2], axis=1).astype(np.uint8)


def sizes_of(t2, S):
    return np.stack([np.bincount(t2[:, r], minlength=S) for r in range(2)]).astype(np.uint64)


def fitness(sizes, n):
    S = sizes.shape[1]
    dev = np.abs(S * sizes.astype(np.int64) - n)
    return int(dev.max()), [int(np.argmax(dev[0])), int(np.argmax(dev[1]))]


def evaluate(x16, c_raw):
    S = c_raw.shape[0]
    return fitness(sizes_of(top2(scores(x16, normalise(c_raw))), S), x16.shape[0])


class Annealer:
    """kmeans.py:96-127 as the header restates it; run(iters) appends to .trace [(F_new, code)]"""

    def __init__(self, orc, x16, S, **config):
        self.orc, self.x16, self.S, self.d, self.n = orc, x16, S, x16.shape[1], x16.shape[0]
        self.cfg = dict(DEFAULTS, **config)
        self.f = {k: np.float32(self.cfg[k]) for k in ("accept_decay", "reject_decay", "reroll_heat", "temperature_cap")}
        self.T = np.float32(self.cfg["temperature0"])
        self.c = np.stack([noise(orc, self.cfg["seed"], s, self.d) for s in range(S)])
        self.last, _ = evaluate(x16, self.c)
        self.li, self.t, self.stopped, self.trace = 0, 0, False, []
        self.stop_num = int(round(self.cfg["stop_fraction"] * 1e6))

    def run(self, iters):
        S, seed = self.S, self.cfg["seed"]
        for _ in range(iters):
            if self.stopped:
                break
            t = self.t + 1
            z = np.stack([noise(self.orc, seed, t * S + s, self.d) for s in range(S)])
            cand = self.c + z * self.T                 # float32 arrays: a rounded product, then a rounded sum
            F, worst = evaluate(self.x16, cand)
            code = 0
            if F < self.last:
                self.c, self.T, self.last, self.li, code = cand, self.T * self.f["accept_decay"], F, 0, 1
            else:
                self.T, self.li = self.T * self.f["reject_decay"], self.li + 1
            if self.li > self.cfg["reroll_after"]:
                self.c = self.c.copy()
                for w in worst:
                    self.c[w] = noise(self.orc, seed, (1 << 40) + t * S + w, self.d)
                self.li, self.T, self.last, code = 0, self.T * self.f["reroll_heat"], F, 2
            if self.last * 1000000 < self.n * self.stop_num:
                self.stopped = True
            else:
                self.T = min(self.f["temperature_cap"], self.T)
            self.trace.append((F, code))
            self.t = t
        return self


def scale_dot_result_f64(x):
    v = np.asarray(x, np.float64) * 4294967296.0
    out = np.zeros(v.shape, np.int64)
    hi, lo, ok = v >= 9223372036854775808.0, v <= -9223372036854775808.0, np.isfinite(v)
    mid = ok & ~hi & ~lo
    out[mid] = np.trunc(v[mid]).astype(np.int64)
    out[hi] = np.iinfo(np.int64).max
    out[lo] = np.iinfo(np.int64).min
    return out


def walk(sc, fudge, counts=None, bal=1):
    """src/dump_processor.rs:438-461 over the float64 scores [n][S]; returns (assignment [n][2] u8, counts [S], bal)"""
    n, S = sc.shape
    counts = np.zeros(S, np.int64) if counts is None else np.asarray(counts, np.int64).copy()
    out = np.empty((n, 2), np.uint8)
    fudge = np.float64(fudge)
    for i in range(n):
        adj = sc[i] - fudge * (counts.astype(np.float64) / np.float64(bal))
        with np.errstate(over="ignore"):
            key = -scale_dot_result_f64(adj)
        first2 = np.argsort(key, kind="stable")[:2]   # smallest keys first, lowest shard index on ties
        out[i] = first2
        counts[first2] += 1
        bal += 1
    return out, counts, bal
