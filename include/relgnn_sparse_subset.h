/*
 * relgnn_sparse_subset.h — C ABI of librelgnn.so, a row subset of sparse node features built on the device (the citation
 * task's `sampled_batches` with `"sparse_features": true`): the CSR of the rows a sampled batch names, the CSR of that
 * subset's transpose, and the long-row plans of both, as relgnn_sparse_features.h takes them.
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * The rule.  Source: a validated CSR matrix [num_rows, num_cols] (rowptr, col, val; relgnn_sparse_features.h).  `nodes`
 * names n of its rows in ANY order, a row possibly more than once; the local id of a row is its position in `nodes`.
 *   subset    sub_rowptr[i + 1] - sub_rowptr[i] = the length of source row nodes[i]; the entries of local row i are the
 *             source row's, in its order (ascending columns), values copied bit for bit.
 *   transpose sub_rowptr_t [num_cols + 1] over the subset's nnz entries; the entries of word f are the local rows that
 *             hold f in ASCENDING local id (a stable sort of the subset's entries on the column), values bit for bit.
 *   plans     for a row-pointer array: rows of more than relgnn_csr_project_split_above() entries in slabs of
 *             relgnn_csr_project_slab(); slabs int32 [S][4] = {row, first entry, one past the last entry, dest} in row
 *             order, dest -1 for a row of one slab, else consecutive workspace rows per row; combos int32 [C][3] =
 *             {row, first ws row, number of ws rows} for the rows of several slabs, in row order.
 * Every array equals, element for element, what the host builds from the same rows (tasks/sparse_features.py: the
 * SparseRows constructor and split_plan); a projection over the result therefore has the bits of one over a host-built
 * container, and forward row i the bits of row nodes[i] of the full matrix's projection.
 *
 * Two steps, because the subset's sizes decide its arrays' shapes:
 *   relgnn_sparse_subset_count  writes sub_rowptr, sub_rowptr_t, the plan offsets of both and eight sizes — nothing whose
 *                               size depends on the subset's nnz.  The caller reads `sizes` back (the ONE read-back),
 *                               allocates, and calls
 *   relgnn_sparse_subset_copy, relgnn_sparse_subset_transpose and relgnn_split_plan_fill (once per structure).
 * sizes int32 [8] = {nnz, slabs, combos, ws rows of the subset; slabs, combos, ws rows of the transpose; 0}.  The row
 *   lengths are added with saturation: nnz == 2^31 - 1 says "2^31 - 1 or more", which no structure here holds (RELGNN_EINVAL
 *   from the fill steps; the other seven sizes mean nothing then).
 *
 * The per-word count uses integer atomic adds on num_cols counters (their result does not depend on order); no float
 * atomic anywhere.  Every store is checked against the capacity the caller passed, a node id outside [0, num_rows) counts
 * as an empty row, every loop is bounded by a row's length, 32 halvings or a launch argument.  A kernel fault is never
 * the error path.
 *
 * Limits (relgnn_sparse_subset_supported): 0 <= n, num_rows, num_cols < 2^31 - 1; the subset's nnz < 2^31 - 1.
 * Workspaces: byte counts from the *_workspace_bytes functions (RELGNN_ENOSPC below them).
 */
#ifndef RELGNN_SPARSE_SUBSET_H_
#define RELGNN_SPARSE_SUBSET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if a subset of n rows of a [num_rows, num_cols] matrix is taken, else 0 */
int relgnn_sparse_subset_supported(int64_t num_rows, int64_t num_cols, int64_t n);

/* ---- the long-row plan of one row-pointer array (callable on its own) ---- */
size_t relgnn_split_plan_workspace_bytes(int64_t num_rows);
/* offsets int32 [num_rows + 1][4] = {slabs, ws rows, combos in front of the row, 0}; sizes int32 [3] = the totals */
int relgnn_split_plan_count(const int32_t* rowptr, int64_t num_rows, int32_t* offsets, int32_t* sizes, void* workspace,
                            size_t workspace_bytes, void* stream);
/* slabs [num_slabs][4] and combos [num_combos][3] from the offsets; num_slabs / num_combos are the capacities */
int relgnn_split_plan_fill(const int32_t* rowptr, int64_t num_rows, const int32_t* offsets, int32_t* slabs,
                           int64_t num_slabs, int32_t* combos, int64_t num_combos, void* stream);

/* ---- the subset ---- */
size_t relgnn_sparse_subset_count_workspace_bytes(int64_t n, int64_t num_cols);
int relgnn_sparse_subset_count(const int32_t* rowptr, const int32_t* col, int64_t num_rows, int64_t num_cols,
                               const int32_t* nodes, int64_t n, int32_t* sub_rowptr, int32_t* sub_rowptr_t,
                               int32_t* plan_offsets, int32_t* plan_offsets_t, int32_t* sizes, void* workspace,
                               size_t workspace_bytes, void* stream);
/* sub_col / sub_val [nnz]: the entries of the named rows */
int relgnn_sparse_subset_copy(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows,
                              const int32_t* nodes, int64_t n, const int32_t* sub_rowptr, int64_t nnz, int32_t* sub_col,
                              float* sub_val, void* stream);
size_t relgnn_sparse_subset_transpose_workspace_bytes(int64_t nnz, int64_t num_cols);
/* sub_col_t / sub_val_t [nnz]: (local row, value) of the subset's entries in (column, local row) order */
int relgnn_sparse_subset_transpose(const int32_t* sub_rowptr, int64_t n, const int32_t* sub_col, const float* sub_val,
                                   int64_t nnz, int64_t num_cols, int32_t* sub_col_t, float* sub_val_t, void* workspace,
                                   size_t workspace_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SPARSE_SUBSET_H_ */
