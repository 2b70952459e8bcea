"""Plain NumPy references for the CSR projection (csrc/csr_project.hip, include/relgnn_sparse_features.h) and the seeded inputs its
tests share.  Nothing here touches the GPU or the package under test.

A structure is a Csr(rowptr, col, val, shape): row r holds the entries [rowptr[r], rowptr[r + 1]), column ids ascending.
    forward64(csr, table)            pre[r, :] = sum_j val[j] * table[col[j], :]
    gradient64(csr, table, y, name)  out[r, :] = sum_j val[j] * (table[col[j], :] * act'(y[col[j], :]))     act' from the OUTPUT y
both float64 and both returning, per output element, k (the number of terms), sum_abs and min_abs (the sum and the smallest of
their magnitudes; inf where k == 0), as tests/seg_reduce_reference.py does.  The weight gradient of out = act(X W) is gradient64 over
transpose(X) with table = dOut and y = out:  dW[f, :] = sum_v X[v, f] * dOut[v, :] * act'(y[v, :]).
A term that is exactly zero (a ReLU derivative of 0) is no term: it is not counted in k, and min_abs does not see it.

Bounds (u = 2^-24; the kernel computes every product and every add in float32, rounded separately):

  linear forward    bound(k, sum_abs) = (k + 3) u sum|term|   (seg_reduce_reference.bound).  A float32 sum of k terms rounds at most
                    k times in its adds, each by at most u times a partial sum that sum|term| (1 + k u) bounds; one more rounding
                    is the product val * table.  Two are spare.  The argument does not ask in which order the terms are added, so
                    the long-row split (four partial sums per slab, slabs added in turn) needs no extra term.

  activated forward |act(p^) - act(p)| <= LIPSCHITZ[name] * |p^ - p| <= LIPSCHITZ[name] * bound(k, sum_abs), and the kernel's own
                    evaluation of act adds ACT_ALLOWANCE * max(1, |act(p)|) (what tests/test_gpu_activations.py holds act_fwd to):
                        forward_tolerance = LIPSCHITZ[name] * bound + ACT_ALLOWANCE * max(1, |act|)
                    This holds where p^ and p lie on the same side of a kink; the inputs below keep every pre-activation farther
                    from 0 than preactivation_margin() (bound plus four float32 steps), so it holds for EVERY element.

  gradient          a term is val * (t * d) with d = act'(y) evaluated in float32 from the float32 y both sides read.  Against the
                    linear term that is one more rounded product, (k + 4) u sum|term|, and the error of d itself: at most two
                    roundings (1 - y * y; y + constant with the constant rounded to float32) of quantities no larger than
                    DACT_SUP[name] = sup |act'|, so |d^ - d| <= 2 u DACT_SUP and the terms move by at most 2 u DACT_SUP sum|val t|:
                        gradient_tolerance = (k + 4) u sum|term| + 2 u DACT_SUP[name] sum|val * t|

Inputs: magnitudes in [0.5, 2] with random signs for values and tables, so that the smallest term of the linear sum is 0.25.  For the
longest row (700 terms) sum|term| is about 700 * 1.25^2 = 1094, bound = 703 u 1094 = 0.046 and 4 * bound = 0.18 < 0.25:
ONE dropped term shows in every element (test_sparse_features_reference_cpu.py verifies the figures).  The y of the gradient keeps
act' in [0.75, 1.76] on all rows that long rows gather (|y| in [0.1, 0.5] for tanh; positive y elsewhere), so the same holds there;
the derivative's other branch (0, 0.2, y + 1, y + 1.758) sits on the last NEGATIVE_ROWS table rows, which only rows of at most 65
entries gather."""
import functools
from collections import namedtuple

import numpy as np

from seg_reduce_reference import ACT_ALLOWANCE, LIPSCHITZ, U, Sum64, act64, bound, dact_from_output64, preactivation_margin

ACTIVATIONS = ("linear", "tanh", "relu", "leaky_relu", "elu", "selu", "gelu")
GRADIENT_ACTIVATIONS = ACTIVATIONS[:6]                 # those whose derivative the output determines, and linear
DACT_SUP = {"linear": 1.0, "tanh": 1.0, "relu": 1.0, "leaky_relu": 1.0, "elu": 1.0, "selu": 1.7580993408473768599402175208123}
_LIPSCHITZ = dict(LIPSCHITZ, linear=1.0)

Csr = namedtuple("Csr", "rowptr col val shape")


def row_ids(csr):
    return np.repeat(np.arange(csr.shape[0]), np.diff(csr.rowptr))


def transpose(csr):
    """The transposed structure: entries by (column, row), a stable sort on the column — the rows of a column stay ascending —
    and the values permuted with them."""
    order = np.argsort(csr.col, kind="stable")
    rowptr = np.zeros(csr.shape[1] + 1, np.int64)
    np.cumsum(np.bincount(csr.col, minlength=csr.shape[1]), out=rowptr[1:])
    return Csr(rowptr, row_ids(csr)[order], csr.val[order], (csr.shape[1], csr.shape[0]))


def dense64(csr):
    out = np.zeros(csr.shape)
    out[row_ids(csr), csr.col] = csr.val
    return out


def _sum_rows(csr, terms):
    """out[r] = sum of terms[j] over the entries j of row r, with k, sum|term| and min|term| per element over the non-zero terms."""
    R, n = csr.shape[0], terms.shape[1]
    value, sum_abs, k = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R, n))
    min_abs = np.full((R, n), np.inf)
    rows = np.flatnonzero(np.diff(csr.rowptr) > 0)
    if len(rows):
        starts = csr.rowptr[rows]
        a = np.abs(terms)
        value[rows] = np.add.reduceat(terms, starts, axis=0)
        sum_abs[rows] = np.add.reduceat(a, starts, axis=0)
        k[rows] = np.add.reduceat((a > 0).astype(np.float64), starts, axis=0)
        min_abs[rows] = np.minimum.reduceat(np.where(a > 0, a, np.inf), starts, axis=0)
    return Sum64(value, k, sum_abs, min_abs)


def forward64(csr, table):
    """The pre-activation sums, float64."""
    return _sum_rows(csr, csr.val.astype(np.float64)[:, None] * np.asarray(table, np.float64)[csr.col])


def forward_act64(csr, table, name):
    """(act(pre), tolerance per element, the Sum64 of the pre-activation)."""
    pre = forward64(csr, table)
    if name == "linear":
        return pre.value, bound(pre.k, pre.sum_abs), pre
    a, _ = act64(name, pre.value)
    return a, _LIPSCHITZ[name] * bound(pre.k, pre.sum_abs) + ACT_ALLOWANCE * np.maximum(1.0, np.abs(a)), pre


def gradient64(csr, table, y, name):
    """(Sum64 of the terms val * table[col] * act'(y[col]), tolerance per element)."""
    vt = csr.val.astype(np.float64)[:, None] * np.asarray(table, np.float64)[csr.col]
    d = np.ones_like(vt) if name == "linear" else dact_from_output64(name, np.asarray(y, np.float64)[csr.col])
    res = _sum_rows(csr, vt * d)
    extra = 0.0 if name == "linear" else 2.0 * U * DACT_SUP[name] * _sum_rows(csr, np.abs(vt)).sum_abs
    return res, (res.k + 4.0) * U * res.sum_abs + extra


def sequential32(csr, table, y=None, name="linear"):
    """The kernel's arithmetic restated in float32, one term after the other in ascending order: s * (t [* act'(y)]), every product
    and every add rounded on its own.  The pre-activation / the gradient, no epilogue."""
    table = np.asarray(table, np.float32)
    out = np.zeros((csr.shape[0], table.shape[1]), np.float32)
    for r in range(csr.shape[0]):
        acc = np.zeros(table.shape[1], np.float32)
        for j in range(int(csr.rowptr[r]), int(csr.rowptr[r + 1])):
            t = table[csr.col[j]]
            if y is not None and name != "linear":
                t = (t * dact32(name, np.asarray(y, np.float32)[csr.col[j]])).astype(np.float32)
            acc = (acc + (np.float32(csr.val[j]) * t).astype(np.float32)).astype(np.float32)
        out[r] = acc
    return out


def dact32(name, y):
    """dact_from_output of csrc/common.h in float32."""
    one = np.float32(1.0)
    if name == "tanh":
        return (one - (y * y).astype(np.float32)).astype(np.float32)
    if name == "relu":
        return np.where(y > 0, one, np.float32(0.0))
    if name == "leaky_relu":
        return np.where(y > 0, one, np.float32(0.2))
    if name == "elu":
        return np.where(y > 0, one, (y + one).astype(np.float32))
    if name == "selu":
        return np.where(y > 0, np.float32(1.0507009873554804934193349852946), (y + np.float32(DACT_SUP["selu"])).astype(np.float32))
    raise KeyError(name)


# ---- the structure and inputs the tests use ---------------------------------------------------------------------------------------
# Row lengths: the tails of the unroll-by-8 loop (0 .. 17), the 64-entry index batch (63, 64, 65), the split threshold of 128
# (128: the longest row one wave sums; 129, 130: four waves, the last three nearly idle), one slab of 512 exactly, and two slabs
# (513: a second slab of one entry; 700).
SHORT_LENGTHS = (0, 1, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65)
LONG_LENGTHS = ((128, 3), (129, 3), (130, 3), (512, 2), (513, 2), (700, 2))
NUM_TABLE_ROWS = 797                    # an odd count that holds a row of 700 distinct columns
NEGATIVE_ROWS = 40                      # the last table rows: gathered only by rows of at most 65 entries
N_MAX = 320


def _signed(rng, shape, lo=0.5, hi=2.0):
    return (rng.uniform(lo, hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def structure():
    """197 rows over NUM_TABLE_ROWS columns with the lengths above, in a shuffled order."""
    rng = np.random.default_rng(7)
    lengths = np.array([l for l in SHORT_LENGTHS for _ in range(14)] + [l for l, c in LONG_LENGTHS for _ in range(c)])
    rng.shuffle(lengths)
    cols = [np.sort(rng.choice(NUM_TABLE_ROWS if l <= 65 else NUM_TABLE_ROWS - NEGATIVE_ROWS, size=l, replace=False)) for l in lengths]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.int64)
    val = _signed(rng, len(col))
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return Csr(rowptr, col, val, (len(lengths), NUM_TABLE_ROWS))


@functools.lru_cache(maxsize=None)
def tables():
    """(table, dout): two float32 [NUM_TABLE_ROWS, N_MAX] arrays.  `table` is adjusted so that every pre-activation of structure()
    lies farther from 0 than preactivation_margin: an element that does not gets the sign of its row's first term flipped (a move
    of at least 0.5), until none is left.  Columns are independent, so the property holds for the first n columns of any n."""
    rng = np.random.default_rng(8)
    csr = structure()
    table, dout = _signed(rng, (NUM_TABLE_ROWS, N_MAX)), _signed(rng, (NUM_TABLE_ROWS, N_MAX))
    for _ in range(100):
        pre = forward64(csr, table)
        close = (pre.k > 0) & (np.abs(pre.value) <= 2.0 * preactivation_margin(pre))
        if not close.any():
            break
        for r, c in zip(*np.nonzero(close)):
            table[csr.col[csr.rowptr[r]], c] *= np.float32(-1.0)
    else:
        raise AssertionError("the pre-activations could not be moved away from 0")
    table.setflags(write=False)
    dout.setflags(write=False)
    return table, dout


@functools.lru_cache(maxsize=None)
def outputs(name):
    """y float32 [NUM_TABLE_ROWS, N_MAX], a possible output of `name`: tanh: |y| in [0.1, 0.5], act' in [0.75, 0.99]; the others:
    y in [0.5, 2] (act' = 1, selu 1.0507), and on the last NEGATIVE_ROWS rows a random half of the elements negative — relu: -0 or
    0 (act' = 0), leaky_relu: [-0.4, -0.1] (0.2), elu: [-0.25, -0.02] (y + 1), selu: [-0.7, -0.05] (y + 1.758)."""
    rng = np.random.default_rng([9, ACTIVATIONS.index(name)])
    shape = (NUM_TABLE_ROWS, N_MAX)
    if name == "linear":
        y = _signed(rng, shape)
    elif name == "tanh":
        y = _signed(rng, shape, 0.1, 0.5)
    else:
        y = rng.uniform(0.5, 2.0, size=shape).astype(np.float32)
        lo, hi = {"relu": (0.0, 0.0), "leaky_relu": (0.1, 0.4), "elu": (0.02, 0.25), "selu": (0.05, 0.7)}[name]
        neg = -rng.uniform(lo, hi, size=(NEGATIVE_ROWS, N_MAX)).astype(np.float32)
        tail = y[-NEGATIVE_ROWS:]
        y[-NEGATIVE_ROWS:] = np.where(rng.random(tail.shape) < 0.5, neg, tail)
    y.setflags(write=False)
    return y
