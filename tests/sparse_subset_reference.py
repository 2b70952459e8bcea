"""Plain NumPy reference for SparseRows.take_rows (include/relgnn_sparse_subset.h, csrc/sparse_subset.hip) and the seeded structure
its tests share.  Nothing here touches the GPU or the package's device code: the only thing taken from the package is the HOST
function split_plan, which the header names as the definition of the plans.

take_rows(rowptr, col, val, shape, nodes) -> Subset: the CSR of the rows `nodes` names (local id = position, any order, a row
possibly twice), the CSR of its transpose by a stable sort on the column (ascending local ids inside a word), and the long-row plan
of both.
"""
import functools
from collections import namedtuple

import numpy as np

from tf_gnn_samples_amd.tasks.sparse_features import split_plan

Structure = namedtuple("Structure", "rowptr col val slabs combos ws_rows num_cols")
Subset = namedtuple("Subset", "rows transposed shape")
FIELDS = ("rowptr", "col", "val", "slabs", "combos")


def _structure(rowptr, col, val, num_cols):
    slabs, combos, ws_rows = split_plan(rowptr)
    return Structure(rowptr.astype(np.int32), col.astype(np.int32), val.astype(np.float32), slabs, combos, ws_rows, num_cols)


def take_rows(rowptr, col, val, shape, nodes) -> Subset:
    rowptr, col, val, nodes = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float32), np.asarray(nodes, np.int64)
    n, F = len(nodes), int(shape[1])
    pieces = [np.arange(rowptr[v], rowptr[v + 1]) for v in nodes]
    entry = np.concatenate(pieces) if pieces else np.zeros(0, np.int64)
    sub_rowptr = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
    sub_col, sub_val = col[entry.astype(np.int64)], val[entry.astype(np.int64)]
    local_row = np.repeat(np.arange(n), np.diff(sub_rowptr))
    order = np.argsort(sub_col, kind="stable")
    rowptr_t = np.zeros(F + 1, np.int64)
    np.cumsum(np.bincount(sub_col, minlength=F), out=rowptr_t[1:])
    return Subset(_structure(sub_rowptr, sub_col, sub_val, F), _structure(rowptr_t, local_row[order], sub_val[order], n), (n, F))


def compare(got, want: Subset, what: str) -> None:
    """Every array of a SparseRows (on any device) against a Subset, element for element; float32 values as bits."""
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    for side in ("rows", "transposed"):
        g, w = getattr(got, side), getattr(want, side)
        assert (g.ws_rows, g.num_cols) == (w.ws_rows, w.num_cols), (what, side, g.ws_rows, w.ws_rows, g.num_cols, w.num_cols)
        for field in FIELDS:
            a, b = getattr(g, field).cpu().numpy(), getattr(w, field)
            assert a.dtype == b.dtype and a.shape == b.shape, (what, side, field, a.dtype, b.dtype, a.shape, b.shape)
            same = np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)
            assert same, "%s: %s.%s differs at %s" % (what, side, field, np.argwhere(a != b)[:5].tolist())


# ---- the structure the tests share ------------------------------------------------------------------------------------------------
V, F = 1300, 800
ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 130, 512, 513, 700)
# word -> how many nodes hold it: the transposed rows of take_rows(arange(V)) (word 0 is in no row)
WORD_NODES = {0: 0, 1: 1, 2: 128, 3: 129, 4: 512, 5: 513, 6: 1025, 7: 513}
FIRST_PLAIN_WORD = 20                    # words 8 .. 19 stay empty too; the rows are filled from [20, F)


def _signed(rng, shape, lo=0.5, hi=2.0):
    return (rng.uniform(lo, hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def structure():
    """(rowptr, col, val) of a [V, F] matrix.  Nodes 1 .. 49 have no entry, node 0 holds word 1 alone, nodes 50 .. 99 one plain word;
    the nodes from 100 on hold the counted words (word 6: nodes 100 .. 1124; word 7: the 513 EVEN nodes among them, so that every
    second node gives 513 as well; words 2 .. 5: a random choice) and are filled with plain words up to their length: three rows each
    of 128, 129 and 130 entries, two each of 512, 513 and 700, six each of 63, 64 and 65, the others 8."""
    rng = np.random.default_rng(11)
    rest = np.arange(100, V)
    holders = {1: np.array([0]), 6: np.arange(100, 1125), 7: np.arange(100, 1125, 2)}
    for word in (2, 3, 4, 5):
        holders[word] = np.sort(rng.choice(rest, size=WORD_NODES[word], replace=False))
    assert all(len(holders[w]) == c for w, c in WORD_NODES.items() if c)
    counted = [[] for _ in range(V)]
    for word in sorted(holders):
        for v in holders[word]:
            counted[v].append(word)
    lengths = np.full(V, 8)
    lengths[:50], lengths[50:100], lengths[0] = 0, 1, 1
    special = [l for l, c in ((128, 3), (129, 3), (130, 3), (512, 2), (513, 2), (700, 2), (63, 6), (64, 6), (65, 6)) for _ in range(c)]
    lengths[rng.choice(rest, size=len(special), replace=False)] = special
    rows = []
    for v in range(V):
        plain = max(0, int(lengths[v]) - len(counted[v]))
        rows.append(np.array(counted[v] + np.sort(rng.choice(np.arange(FIRST_PLAIN_WORD, F), size=plain, replace=False)).tolist(), np.int64))
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows)
    val = _signed(rng, len(col))
    assert set(ROW_LENGTHS) <= set(np.diff(rowptr).tolist())
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val


@functools.lru_cache(maxsize=None)
def subsets():
    """name -> int32 node list."""
    rowptr, _, _ = structure()
    lengths = np.diff(rowptr)
    rng = np.random.default_rng(12)
    long_rows = np.flatnonzero(lengths > 65)                                # every row of 128 entries and more, and 400 others, shuffled
    twice = rng.permutation(np.concatenate([long_rows, rng.choice(np.flatnonzero(lengths <= 65), size=400, replace=False)]))
    twice = np.insert(twice, 7, twice[300])                                 # a node named twice, far apart
    named = {
        "one node": np.array([int(np.flatnonzero(lengths == 700)[0])]),
        "all": np.arange(V),
        "every second": np.arange(0, V, 2),
        "descending": np.arange(V)[::-1],
        "a node twice": twice,
        "few words": np.array([60, 0, 75, 50]),                             # four entries in all: most words stay empty
        "empty rows only": np.array([49, 1, 17, 17, 30]),
    }
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in named.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    rowptr, col, val = structure()
    return take_rows(rowptr, col, val, (V, F), subsets()[name])
