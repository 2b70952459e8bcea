"""NumPy float32 restatement of the dense Adam element update (csrc/adam_element.h) and of the row-deferred scheme of
include/relgnn_sparse_update.h: stamps, the table of step sizes, the replay with g = +0, the forced flush when the table is full.

Every operation is one IEEE float32 operation (NumPy keeps subnormals and rounds sqrt and the quotient correctly, as the kernels
do), in the order the device function writes them, so finite results are compared bit for bit.  NaN PAYLOADS are the one thing a
host cannot restate (an x86 invalid operation gives a negative quiet NaN): the tests compare those against the dense launch."""
import numpy as np

F32 = np.float32
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)
ONE = F32(1.0)


def step_size(lr: float, t: int) -> np.float32:
    """lr_t of step t as the launches receive it: formed in double on the host, rounded once to float32."""
    return F32(lr * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t))


def clip_scale(norm, clip) -> np.float32:
    """clip > 0 ? clip / fmaxf(norm, clip) : 1 (fmaxf: a NaN norm gives clip)."""
    norm, clip = F32(norm), F32(clip)
    if not clip > 0:
        return ONE
    with np.errstate(all="ignore"):
        return clip / (clip if np.isnan(norm) else max(norm, clip))


def adam_element(p, gi, m, v, lr_t):
    """-> (p, m, v) after one step on float32 arrays; gi is the clipped gradient."""
    p, gi, m, v, lr_t = (np.asarray(a, F32) for a in (p, gi, m, v, lr_t))
    with np.errstate(all="ignore"):
        mi = B1 * m + (ONE - B1) * gi
        vi = B2 * v + (ONE - B2) * (gi * gi)
        return p - lr_t * mi / (np.sqrt(vi) + EPS), mi, vi


def shortcut_element(p, gi, m, v, lr_t):
    """The replay one might write instead (decay the slots, no gradient terms): NOT the same rule, see the CPU test."""
    p, m, v, lr_t = (np.asarray(a, F32) for a in (p, m, v, lr_t))
    with np.errstate(all="ignore"):
        mi, vi = B1 * m, B2 * v
        return p - lr_t * mi / (np.sqrt(vi) + EPS), mi, vi


class Dense:
    """Dense Adam over [F, n] arrays: every row every step."""

    def __init__(self, p, m, v, t=0):
        self.p, self.m, self.v = (np.array(a, F32) for a in (p, m, v))
        self.t = int(t)

    def step(self, g, lr_t, scale=ONE):
        self.t += 1
        with np.errstate(all="ignore"):
            gi = np.asarray(g, F32) * F32(scale)
        self.p, self.m, self.v = adam_element(self.p, gi, self.m, self.v, F32(lr_t))


class Deferred:
    """The scheme of models/optimizer.py over the same arrays.  `named` is a bool [F] (None: every row)."""

    def __init__(self, p, m, v, capacity, t=0, replay=adam_element):
        self.p, self.m, self.v = (np.array(a, F32) for a in (p, m, v))
        self.t = self.base = int(t)
        self.capacity = int(capacity)
        self.stamps = np.full(len(self.p), self.t, np.int32)
        self.step_sizes = np.zeros(self.capacity, F32)
        self._replay = replay
        self.forced_flushes = 0
        self.gaps_seen = set()             # how many steps a row was behind whenever it was replayed

    def _rows(self, named):
        return range(len(self.p)) if named is None else np.flatnonzero(named)

    def _replay_rows(self, named, upto):
        zero = np.zeros(self.p.shape[1], F32)
        for f in self._rows(named):
            self.gaps_seen.add(max(0, upto - max(int(self.stamps[f]), self.base)))
            for s in range(max(int(self.stamps[f]), self.base) + 1, upto + 1):
                self.p[f], self.m[f], self.v[f] = self._replay(self.p[f], zero, self.m[f], self.v[f], self.step_sizes[s - self.base - 1])
            self.stamps[f] = max(int(self.stamps[f]), upto)

    def catch_up(self, named):
        self._replay_rows(named, self.t)

    def flush(self):
        self._replay_rows(None, self.t)
        self.base = self.t

    def pending_rows(self) -> int:
        return int((self.stamps < self.t).sum())

    def step(self, named, g, lr_t, scale=ONE):
        if self.t - self.base == self.capacity:
            self.flush()
            self.forced_flushes += 1
        self.t += 1
        self.step_sizes[self.t - self.base - 1] = F32(lr_t)
        self._replay_rows(named, self.t - 1)
        rows = list(self._rows(named))
        with np.errstate(all="ignore"):
            gi = np.asarray(g, F32)[rows] * F32(scale)
        self.p[rows], self.m[rows], self.v[rows] = adam_element(self.p[rows], gi, self.m[rows], self.v[rows], F32(lr_t))
        self.stamps[rows] = self.t


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F32).view(np.uint32)


def special_values(rng, F, n):
    """(p, m, v) float32 [F, n] of ordinary magnitudes with the values the scheme could get wrong planted in rows 0-3: m = -0 with
    p = -0, a subnormal m, v = 0, p = +0."""
    p = (rng.standard_normal((F, n)) * 0.1).astype(F32)
    m = (rng.standard_normal((F, n)) * 1e-3).astype(F32)
    v = (rng.random((F, n)) * 1e-5).astype(F32)
    p[0], m[0] = F32(-0.0), F32(-0.0)
    m[1] = F32(1e-41) * np.where(np.arange(n) % 2, 1, -1).astype(F32)
    v[2], m[2] = 0, 0
    p[3] = F32(0.0)
    v[0, ::2] = 0
    return p, m, v


def touch_patterns(F):
    """name -> bool [F]"""
    none, alternating, ends = np.zeros(F, bool), np.arange(F) % 2 == 0, np.zeros(F, bool)
    ends[[0, F - 1]] = True
    return {"none": none, "all": np.ones(F, bool), "alternating": alternating, "first and last": ends}


def rowptr_of(named) -> np.ndarray:
    """An int32 row pointer [F + 1] whose non-empty rows are the named ones (1 to 3 entries each)."""
    named = np.asarray(named, bool)
    return np.concatenate([[0], np.cumsum(np.where(named, 1 + np.arange(len(named)) % 3, 0))]).astype(np.int32)
