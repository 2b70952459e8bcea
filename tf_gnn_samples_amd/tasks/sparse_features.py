"""Sparse node features: a [V, F] float32 matrix as CSR plus its transpose, the operand of ops.csr_rows_project
(csrc/csr_project.hip, include/relgnn_sparse_features.h).

The citation-network task's `sparse_node_features` mode keeps the bag-of-words features in this container instead of a dense
[V, F] table: the three folds share ONE SparseRows, every device holds one copy of it, and the input projection gathers rows of the
weight matrix.  The transpose (the structure the weight gradient runs over) and the long-row plans of both structures are built once,
on the host, when the container is made; so is the validation the kernels rely on.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib

# The summation order of include/relgnn_sparse_features.h (relgnn_csr_project_split_above / relgnn_csr_project_slab; the library
# is not loaded to build a container, tests/test_gpu_sparse_features.py holds the two against each other)
SPLIT_ABOVE = 128
SLAB = 512
_INT32_MAX = 2 ** 31 - 1


def split_plan(rowptr: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """(slabs int32 [S, 4], combos int32 [C, 3], workspace rows) of include/relgnn_sparse_features.h for one row-pointer array:
    rows of more than SPLIT_ABOVE entries in slabs of SLAB; a row of one slab is written directly (dest -1), the slabs of a longer
    row go to consecutive workspace rows."""
    rowptr = np.asarray(rowptr, np.int64)
    length = np.diff(rowptr)
    long_rows = np.flatnonzero(length > SPLIT_ABOVE)
    if not len(long_rows):
        return np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), 0
    per_row = (length[long_rows] + SLAB - 1) // SLAB
    row_of_slab = np.repeat(long_rows, per_row)
    first_slab = np.concatenate([[0], np.cumsum(per_row)])[:-1]
    index_in_row = np.arange(int(per_row.sum())) - np.repeat(first_slab, per_row)
    begin = rowptr[row_of_slab] + index_in_row * SLAB
    end = np.minimum(begin + SLAB, rowptr[row_of_slab + 1])
    several = per_row > 1
    ws_first = np.concatenate([[0], np.cumsum(np.where(several, per_row, 0))])[:-1]
    dest = np.where(np.repeat(several, per_row), np.repeat(ws_first, per_row) + index_in_row, -1)
    slabs = np.stack([row_of_slab, begin, end, dest], axis=1).astype(np.int32)
    combos = np.stack([long_rows[several], ws_first[several], per_row[several]], axis=1).astype(np.int32).reshape(-1, 3)
    return np.ascontiguousarray(slabs), np.ascontiguousarray(combos), int(per_row[several].sum())


class CsrStructure:
    """rowptr int32 [R + 1], col int32 [nnz], val float32 [nnz] and the long-row plan, as tensors of one device."""

    def __init__(self, rowptr, col, val, slabs, combos, ws_rows: int, num_cols: int):
        self.rowptr, self.col, self.val, self.slabs, self.combos = rowptr, col, val, slabs, combos
        self.ws_rows, self.num_cols = int(ws_rows), int(num_cols)

    @property
    def num_rows(self) -> int:
        return int(self.rowptr.shape[0]) - 1

    @property
    def nnz(self) -> int:
        return int(self.col.shape[0])

    def row_ids(self) -> torch.Tensor:
        """The row of every entry, int64 [nnz] (the torch composition's index_add_ target)."""
        counts = (self.rowptr[1:] - self.rowptr[:-1]).long()
        return torch.repeat_interleave(torch.arange(self.num_rows, device=self.rowptr.device), counts)

    def to(self, device) -> "CsrStructure":
        move = lambda t: t.to(device)
        return CsrStructure(move(self.rowptr), move(self.col), move(self.val), move(self.slabs), move(self.combos), self.ws_rows,
                            self.num_cols)


class NamedRows:
    """The words a container's transposed structure names (include/relgnn_sparse_gradient.h): words int32 [T] ascending, slot int32
    [F + 1] (slot[words[t]] == t, slot[F] == T) and `structure`, the transposed structure as a CSR of T rows — it SHARES col and val
    with it (rows without entries hold none, so the entries are contiguous already), rowptr without its repeats, the long-row plan
    with its rows mapped through slot.  ops.csr_rows_project's gradient over `structure` is [T, n]: row t has the bits of row
    words[t] of the gradient over the transposed structure."""

    def __init__(self, words, slot, structure: CsrStructure):
        self.words, self.slot, self.structure = words, slot, structure

    @property
    def count(self) -> int:
        return int(self.words.shape[0])

    def tensors(self):
        s = self.structure
        return (self.words, self.slot, s.rowptr, s.slabs, s.combos)

    def to(self, device) -> "NamedRows":
        return NamedRows(self.words.to(device), self.slot.to(device), self.structure.to(device))


def named_rows_of(transposed: CsrStructure) -> NamedRows:
    """NamedRows of a transposed structure, in NumPy (what a host-built container uses; the device arrays of
    csrc/sparse_gradient.hip equal these element for element)."""
    rowptr = transposed.rowptr.cpu().numpy().astype(np.int64)
    named = np.diff(rowptr) > 0
    words = np.flatnonzero(named)
    slot = np.zeros(len(rowptr), np.int64)
    np.cumsum(named, out=slot[1:])
    rowptr_c = np.concatenate([rowptr[words], rowptr[-1:]])
    slabs, combos = transposed.slabs.cpu().numpy().copy(), transposed.combos.cpu().numpy().copy()
    if len(slabs):
        slabs[:, 0] = slot[slabs[:, 0]]
    if len(combos):
        combos[:, 0] = slot[combos[:, 0]]
    dev = transposed.rowptr.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    return NamedRows(t(words), t(slot), CsrStructure(t(rowptr_c), transposed.col, transposed.val, t(slabs), t(combos),
                                                      transposed.ws_rows, transposed.num_cols))


def _validated(rowptr, col, val, shape):
    V, F = int(shape[0]), int(shape[1])
    rowptr, col, val = np.asarray(rowptr), np.asarray(col), np.asarray(val)
    if V < 0 or F < 0:
        raise ValueError("SparseRows: negative shape %r" % (shape,))
    if rowptr.ndim != 1 or col.ndim != 1 or val.ndim != 1 or rowptr.dtype.kind not in "iu" or col.dtype.kind not in "iu":
        raise ValueError("SparseRows: rowptr, col and val are one-dimensional, rowptr and col integers")
    if len(rowptr) != V + 1:
        raise ValueError("SparseRows: rowptr has %d entries, expected %d" % (len(rowptr), V + 1))
    nnz = len(col)
    if len(val) != nnz:
        raise ValueError("SparseRows: %d column ids but %d values" % (nnz, len(val)))
    if nnz >= _INT32_MAX or V >= _INT32_MAX or F >= _INT32_MAX:
        raise ValueError("SparseRows: the structure is indexed with 32 bits (nnz, rows and columns below 2^31 - 1)")
    rowptr = rowptr.astype(np.int64)
    if rowptr[0] != 0 or rowptr[-1] != nnz or (np.diff(rowptr) < 0).any():
        raise ValueError("SparseRows: rowptr must rise from 0 to nnz = %d without a step down" % nnz)
    col = col.astype(np.int64)
    if nnz and (col.min() < 0 or col.max() >= F):
        raise ValueError("SparseRows: column id outside [0, %d)" % F)
    if nnz > 1:
        rising = col[1:] > col[:-1]
        rising[rowptr[1:-1][(rowptr[1:-1] > 0) & (rowptr[1:-1] < nnz)] - 1] = True      # the first entry of a row follows another row
        if not rising.all():
            raise ValueError("SparseRows: the column ids of a row must be sorted and unique")
    val = np.ascontiguousarray(val, dtype=np.float32)
    if (val == 0).any():
        raise ValueError("SparseRows: explicit zeros are not stored (eliminate_zeros)")
    return rowptr, col, val


def _structure(rowptr, col, val, num_cols) -> CsrStructure:
    slabs, combos, ws_rows = split_plan(rowptr)
    t = torch.from_numpy                                   # (np.array copies: the container owns its arrays)
    return CsrStructure(t(np.array(rowptr, dtype=np.int32)), t(np.array(col, dtype=np.int32)), t(np.array(val, dtype=np.float32)),
                        t(slabs), t(combos), ws_rows, num_cols)


class PhaseTrace:
    """trace = a list: every call appends (phase, timed event recorded behind it); None: nothing is recorded (scripts/bench_*sampl*)."""
    trace = None

    def _mark(self, phase: str) -> None:
        if self.trace is not None:
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            self.trace.append((phase, event))


class SparseRows(PhaseTrace):                # (the phases of a take_rows: scripts/bench_sparse_sampling.py)
    """A [V, F] float32 matrix in CSR (`rows`) and in CSR of its transpose (`transposed`: F rows over V columns), both with
    ascending ids inside a row and built once on the host with a stable sort.  The structure is validated here — monotone rowptr,
    0 <= col < F, sorted and unique columns per row, no explicit zeros — and raises ValueError: the kernels trust what they read."""

    requires_grad = False            # the features are data
    _named = None                    # named_rows(): built when asked

    def __init__(self, rowptr, col, val, shape, _structures=None):
        self.shape = (int(shape[0]), int(shape[1]))
        if _structures is not None:                       # (to(): already validated)
            self.rows, self.transposed = _structures
            return
        rowptr, col, val = _validated(rowptr, col, val, shape)
        V, F = self.shape
        self.rows = _structure(rowptr, col, val, F)
        # the transpose: entries by (column, row); a stable sort on the column keeps the rows of a column ascending
        order = np.argsort(col, kind="stable")
        row_of = np.repeat(np.arange(V, dtype=np.int64), np.diff(rowptr))
        rowptr_t = np.zeros(F + 1, np.int64)
        np.cumsum(np.bincount(col, minlength=F), out=rowptr_t[1:])
        self.transposed = _structure(rowptr_t, row_of[order], val[order], V)

    # ---- makers ----
    @classmethod
    def from_scipy(cls, matrix) -> "SparseRows":
        """Any scipy sparse matrix: duplicates summed, explicit zeros dropped, columns sorted, values cast to float32."""
        import scipy.sparse as sp
        m = sp.csr_matrix(matrix, copy=True)
        m.sum_duplicates()
        m = m.astype(np.float32)
        m.eliminate_zeros()
        m.sort_indices()
        return cls(m.indptr, m.indices, m.data, m.shape)

    @classmethod
    def row_normalised(cls, matrix) -> "SparseRows":
        """tasks.citation_network_task.row_normalise without the dense table: the same diags(reciprocal).dot(features), kept
        sparse, then eliminate_zeros, sort_indices and the cast to float32 — every stored value is the dense table's entry bit
        for bit."""
        import scipy.sparse as sp
        row_sum = np.array(matrix.sum(1))
        with np.errstate(divide="ignore"):
            reciprocal = np.power(row_sum, -1).flatten()
        reciprocal[np.isinf(reciprocal)] = 0.
        m = sp.csr_matrix(sp.diags(reciprocal).dot(matrix))
        m.sum_duplicates()
        m.eliminate_zeros()
        m.sort_indices()
        m = m.astype(np.float32)
        m.eliminate_zeros()                                # (a value that the cast flushed to zero is not stored either)
        return cls(m.indptr, m.indices, m.data, m.shape)

    # ---- what a feature table answers ----
    def __len__(self) -> int:
        return self.shape[0]

    @property
    def nnz(self) -> int:
        return self.rows.nnz

    @property
    def device(self) -> torch.device:
        return self.rows.val.device

    @property
    def dtype(self) -> torch.dtype:
        return self.rows.val.dtype

    @property
    def is_cuda(self) -> bool:
        return self.rows.val.is_cuda

    def to(self, device) -> "SparseRows":
        if torch.device(device) == self.device:
            return self
        moved = SparseRows(None, None, None, self.shape, _structures=(self.rows.to(device), self.transposed.to(device)))
        if self._named is not None:                       # (col and val stay shared with the moved transposed structure)
            n, t = self._named.to(device), moved.transposed
            moved._named = NamedRows(n.words, n.slot, CsrStructure(n.structure.rowptr, t.col, t.val, n.structure.slabs,
                                                                   n.structure.combos, t.ws_rows, t.num_cols))
        return moved

    def to_dense(self) -> torch.Tensor:
        """The [V, F] float32 table on the container's device."""
        out = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        if self.nnz:
            out[self.rows.row_ids(), self.rows.col.long()] = self.rows.val
        return out

    def record_stream(self, stream) -> None:
        pass                                               # (a fold-lifetime table: never returned to the allocator under a batch)

    # ---- the words the container names (include/relgnn_sparse_gradient.h) ----
    @property
    def has_named_rows(self) -> bool:
        return self._named is not None

    def named_rows(self) -> NamedRows:
        """The NamedRows of this container, built once: a GPU container runs csrc/sparse_gradient.hip (a read-back of T;
        take_rows(named_rows=True) folds it into its own), a CPU container NumPy."""
        if self._named is None:
            if self.is_cuda:
                with torch.cuda.device(self.device):
                    slot, count = self._named_rows_count(self.transposed.rowptr, None)
                    self._named = self._named_rows_fill(self.transposed, slot, int(count.item()))
            else:
                self._named = named_rows_of(self.transposed)
        return self._named

    def _named_rows_count(self, rowptr_t: torch.Tensor, sizes: Optional[torch.Tensor]):
        """The count step over a transposed row pointer: (slot, the int32 tensor that T is written to — sizes[8:9] when `sizes`,
        the buffer of take_rows' one read-back, is given)."""
        lib, dev, F = _lib.load_library(), rowptr_t.device, int(rowptr_t.shape[0]) - 1
        slot = torch.empty(F + 1, dtype=torch.int32, device=dev)
        count = sizes[8:9] if sizes is not None else torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = lib.relgnn_named_rows_workspace_bytes(F)
        ws = _lib.scratch(nbytes, dev)
        _lib.launch("relgnn_named_rows_count", _lib.ptr(rowptr_t), F, _lib.ptr(slot), count.data_ptr(), _lib.ptr(ws), nbytes)
        return slot, count

    @staticmethod
    def _named_rows_fill(transposed: CsrStructure, slot: torch.Tensor, T: int) -> NamedRows:
        dev, F = slot.device, int(slot.shape[0]) - 1
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        num_slabs, num_combos = int(transposed.slabs.shape[0]), int(transposed.combos.shape[0])
        if T == 0:                                            # nothing named: no entries, no plan, nothing to launch
            return NamedRows(i32(0), slot, CsrStructure(torch.zeros(1, dtype=torch.int32, device=dev), transposed.col, transposed.val,
                                                        i32(0, 4), i32(0, 3), 0, transposed.num_cols))
        words, rowptr_c, slabs, combos = i32(T), i32(T + 1), i32(num_slabs, 4), i32(num_combos, 3)
        _lib.launch("relgnn_named_rows_fill", _lib.ptr(transposed.rowptr), F, _lib.ptr(slot), T, _lib.ptr(words), _lib.ptr(rowptr_c),
                    _lib.ptr(transposed.slabs) if num_slabs else None, _lib.ptr(slabs) if num_slabs else None, num_slabs,
                    _lib.ptr(transposed.combos) if num_combos else None, _lib.ptr(combos) if num_combos else None, num_combos)
        return NamedRows(words, slot, CsrStructure(rowptr_c, transposed.col, transposed.val, slabs, combos, transposed.ws_rows,
                                                   transposed.num_cols))

    # ---- a row subset (include/relgnn_sparse_subset.h) ----
    def take_rows(self, nodes, validated: bool = False, named_rows: bool = False) -> "SparseRows":
        """The [n, F] container of the rows `nodes` names (one-dimensional int32 tensor or array, any order, a row possibly twice;
        local id = position), on this container's device, with every array equal to what SparseRows(rowptr, col, val, (n, F))
        builds from the same rows.  A GPU container runs csrc/sparse_subset.hip (one read-back of eight sizes), a CPU container the
        host constructor; ROUTES["take_rows"] says which.  validated=True trusts `nodes` (the sampler's own output).
        named_rows=True builds the subset's NamedRows too (named_rows() then costs nothing): on the GPU its count rides in the
        same read-back, one int behind the eight sizes."""
        if not validated:
            host = nodes.detach().cpu().numpy() if torch.is_tensor(nodes) else np.asarray(nodes)
            if host.ndim != 1 or host.dtype != np.int32:
                raise ValueError("take_rows: nodes must be a one-dimensional int32 array")
            if len(host) and (host.min() < 0 or host.max() >= self.shape[0]):
                raise ValueError("take_rows: row id outside [0, %d)" % self.shape[0])
        n, F = int(nodes.shape[0]), self.shape[1]
        if not take_rows_supported(self.shape[0], F, n):
            raise ValueError("take_rows: %d rows of a %r matrix are outside what the subset kernels index with 32 bits "
                             "(take_rows_supported)" % (n, self.shape))
        if not self.is_cuda or n == 0:
            ROUTES["take_rows"] = "host"
            return self._take_rows_host(nodes.detach().cpu().numpy() if torch.is_tensor(nodes) else np.asarray(nodes), named_rows)
        ROUTES["take_rows"] = "hip"
        nodes = nodes.to(self.device).contiguous() if torch.is_tensor(nodes) else torch.as_tensor(np.ascontiguousarray(nodes), device=self.device)
        with torch.cuda.device(self.device):
            return self._take_rows_device(nodes, n, named_rows)

    def _take_rows_host(self, nodes: np.ndarray, named_rows: bool = False) -> "SparseRows":
        s = self.rows
        rowptr, nodes = s.rowptr.cpu().numpy().astype(np.int64), nodes.astype(np.int64)
        length = rowptr[nodes + 1] - rowptr[nodes]
        sub_rowptr = np.zeros(len(nodes) + 1, np.int64)
        np.cumsum(length, out=sub_rowptr[1:])
        if sub_rowptr[-1] >= _INT32_MAX:
            raise ValueError("take_rows: the subset holds %d entries; the structure is indexed with 32 bits" % sub_rowptr[-1])
        entry = np.repeat(rowptr[nodes] - sub_rowptr[:-1], length) + np.arange(sub_rowptr[-1])      # the source entry of every entry
        taken = SparseRows(sub_rowptr, s.col.cpu().numpy()[entry], s.val.cpu().numpy()[entry], (len(nodes), self.shape[1]))
        if named_rows:
            taken.named_rows()                                # (in NumPy, before the move)
        return _PerBatchRows.of(taken.to(self.device))

    def _take_rows_device(self, nodes: torch.Tensor, n: int, named_rows: bool = False) -> "SparseRows":
        lib, s, dev = _lib.load_library(), self.rows, self.device
        V, F = self.shape
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        sub_rowptr, sub_rowptr_t, offsets, offsets_t, sizes = i32(n + 1), i32(F + 1), i32(n + 1, 4), i32(F + 1, 4), i32(9 if named_rows else 8)
        nbytes = lib.relgnn_sparse_subset_count_workspace_bytes(n, F)
        ws = _lib.scratch(nbytes, dev)
        self._mark("start")
        _lib.launch("relgnn_sparse_subset_count", _lib.ptr(s.rowptr), _lib.ptr(s.col) if s.nnz else None, V, F, _lib.ptr(nodes), n,
                    _lib.ptr(sub_rowptr), _lib.ptr(sub_rowptr_t), _lib.ptr(offsets), _lib.ptr(offsets_t), _lib.ptr(sizes), _lib.ptr(ws),
                    nbytes)
        if named_rows:                                        # T goes to sizes[8]: the same read-back
            slot, _ = self._named_rows_count(sub_rowptr_t, sizes)
        self._mark("count")
        host_sizes = sizes.tolist()                           # the one read-back: everything below is sized by these
        nnz, *plan_sizes = host_sizes[:7]
        self._mark("readback")
        if nnz >= _INT32_MAX:
            raise ValueError("take_rows: the subset holds 2^31 - 1 entries or more; the structure is indexed with 32 bits")
        sub_col, sub_val = i32(nnz), torch.empty(nnz, dtype=torch.float32, device=dev)
        sub_col_t, sub_val_t = i32(nnz), torch.empty(nnz, dtype=torch.float32, device=dev)
        if nnz:
            _lib.launch("relgnn_sparse_subset_copy", _lib.ptr(s.rowptr), _lib.ptr(s.col), _lib.ptr(s.val), V, _lib.ptr(nodes), n,
                        _lib.ptr(sub_rowptr), nnz, _lib.ptr(sub_col), _lib.ptr(sub_val))
        self._mark("copy")
        if nnz:
            nbytes = lib.relgnn_sparse_subset_transpose_workspace_bytes(nnz, F)
            ws = _lib.scratch(nbytes, dev)
            _lib.launch("relgnn_sparse_subset_transpose", _lib.ptr(sub_rowptr), n, _lib.ptr(sub_col), _lib.ptr(sub_val), nnz, F,
                        _lib.ptr(sub_col_t), _lib.ptr(sub_val_t), _lib.ptr(ws), nbytes)
        self._mark("transpose")
        structures = []
        for rowptr, off, col, val, (num_slabs, num_combos, ws_rows), cols in ((sub_rowptr, offsets, sub_col, sub_val, plan_sizes[:3], F),
                                                                              (sub_rowptr_t, offsets_t, sub_col_t, sub_val_t, plan_sizes[3:], n)):
            slabs, combos = i32(num_slabs, 4), i32(num_combos, 3)
            if num_slabs:
                _lib.launch("relgnn_split_plan_fill", _lib.ptr(rowptr), int(rowptr.shape[0]) - 1, _lib.ptr(off), _lib.ptr(slabs), num_slabs,
                            _lib.ptr(combos) if num_combos else None, num_combos)
            structures.append(CsrStructure(rowptr, col, val, slabs, combos, ws_rows, cols))
        self._mark("plans")
        taken = _PerBatchRows(None, None, None, (n, F), _structures=tuple(structures))
        if named_rows:
            taken._named = self._named_rows_fill(taken.transposed, slot, host_sizes[8])
            self._mark("named")
        return taken


class _PerBatchRows(SparseRows):
    """What take_rows returns: a container that lives as long as its batch, so a consumer on another stream records its tensors."""

    @classmethod
    def of(cls, rows: SparseRows) -> "_PerBatchRows":
        taken = cls(None, None, None, rows.shape, _structures=(rows.rows, rows.transposed))
        taken._named = rows._named
        return taken

    def to(self, device) -> "SparseRows":
        return self if torch.device(device) == self.device else _PerBatchRows.of(super().to(device))

    def record_stream(self, stream) -> None:
        if not self.is_cuda:
            return
        for s in (self.rows, self.transposed):
            for t in (s.rowptr, s.col, s.val, s.slabs, s.combos):
                t.record_stream(stream)
        if self._named is not None:
            for t in self._named.tensors():
                t.record_stream(stream)


ROUTES = {"take_rows": None}         # which implementation the last SparseRows.take_rows took: "hip" or "host"


def take_rows_supported(num_rows: int, num_cols: int, n: int) -> bool:
    """What relgnn_sparse_subset_supported takes (restated: asked before the library is loaded); the subset's own nnz must stay
    below 2^31 - 1 too, which only the count step knows."""
    return all(0 <= x < _INT32_MAX for x in (int(num_rows), int(num_cols), int(n)))


def node_stand_in(num_nodes: int) -> np.ndarray:
    """The per-node payload the input pipelines carry under `initial_node_features` in place of the table: float32 [V, 1] zeros
    (the pipelines read its length for the node count, DeviceBatch.wait_ready its device)."""
    return np.zeros((int(num_nodes), 1), np.float32)


def random_rows(rng, num_rows: int, num_cols: int, per_row, draw=None) -> Tuple[np.ndarray, np.ndarray]:
    """(rowptr, col) of a structure whose row r holds per_row[r] draws of a column id (uniform, or draw(size) -> ids), ascending,
    a column drawn twice for a row counted once: drawn per entry, never through a [rows, cols] array."""
    per_row = np.asarray(per_row, np.int64)
    row_of = np.repeat(np.arange(num_rows, dtype=np.int64), per_row)
    ids = rng.integers(0, num_cols, size=len(row_of)) if draw is None else np.asarray(draw(len(row_of)), np.int64)
    key = np.unique(row_of * np.int64(num_cols) + ids)
    rowptr = np.zeros(num_rows + 1, np.int64)
    np.cumsum(np.bincount(key // num_cols, minlength=num_rows), out=rowptr[1:])
    return rowptr, key % num_cols


def resident_copy(cache, rows: Optional[SparseRows], device) -> Optional[SparseRows]:
    """The one copy of `rows` on `device`, kept in `cache` (a WeakKeyDictionary: released with the host container)."""
    if rows is None:
        return None
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if rows.device == device:
        return rows
    per_device = cache.setdefault(rows, {})
    if device not in per_device:
        per_device[device] = rows.to(device)
    return per_device[device]
