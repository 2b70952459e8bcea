/*
 * window_block.h — PACKAGE-INTERNAL entry points of librelgnn.so: the block of a window of target rows of ONE graph, cut from the
 * by-target bucketing its RelGraph already holds (tasks/layerwise.py, window_block; DESIGN.md section 3, "Layer-wise evaluation").
 * NOT part of the public C ABI: nothing under include/ declares these, tf_gnn_samples_amd/_lib.py binds them from its table INTERNAL,
 * and they may change with the package.
 *
 * The conventions of include/relgnn_sampling.h hold: every pointer is a DEVICE pointer owned by the caller, `stream` is a hipStream_t
 * passed as void* and the last argument, all work is enqueued asynchronously, every entry point returns an int status
 * (RELGNN_OK == 0) and never throws, nothing is allocated or retained, nothing synchronises, nothing is read back.
 *
 * The graph: V nodes, L edge types, M messages, rowptr_t [V * L + 1] and col_t [M] of its RelGraph (row t * L + l holds the messages
 *   of type l into node t; col_t[p] = source * L + l).  The by-target bucketing is target-major, so the entries of the targets
 *   [first, last) are the ONE slice col_t[entry_base, entry_base + num_entries) with entry_base = rowptr_t[first * L] and
 *   num_entries = rowptr_t[last * L] - entry_base: the caller holds both on the host.  T = last - first.
 * The block: nodes [n] = first .. last - 1, then every source of the slice outside [first, last) in ascending id (local id T + i);
 *   per edge type the list of (source, target) pairs in local ids, type l's entries in the order of the slice (ascending target, a
 *   bucket in its own order, duplicates kept), the lists laid one behind the other in ONE int32 [num_entries, 2] array; degrees
 *   float32 [L, n] = the bucket lengths of the target rows, 0 behind them.
 *
 * relgnn_window_block_count: counts[l * T + i] = the length of bucket (first + i, l) and a closing 0, offsets = their exclusive sums
 *   (offsets[l * T + i] is where bucket (first + i, l) begins in the edge array), totals[0 .. L) = the entries per type, totals[L] =
 *   all of them; then ONE flat pass over the slice (nothing when num_entries == 0) that stamps every source outside the window with
 *   1.  The caller compacts the stamps (relgnn_neighbour_sample_compact, value 1) and reads totals[0 .. L) and the compaction's
 *   count back: the one read-back of a window.
 * relgnn_window_block_emit: one flat pass over the slice (nothing when num_entries == 0): an entry finds its row by a binary search in
 *   rowptr_t[first * L .. last * L], its slot is offsets[its bucket] + its position in the bucket, its source's local id the source's
 *   rank in `outside` (a binary search) behind T, or source - first inside the window.  Then nodes, the degree table, and the stamps
 *   of `outside` are cleared: the stamp array is all zero again.
 *
 * Shape of the work: tiles of relgnn_window_block_tile() = 1024 entries, one entry per lane; no loop is bounded by a bucket's length.
 *   No atomics, no spin-wait, no hand-over between workgroups: a stamp is written with a plain store of the one value every writer
 *   writes, and the result is a pure function of the arguments on any stream.
 * The kernels trust no size: every store is checked against its buffer's length and every load of col_t, rowptr_t, stamp and
 *   `outside` against its array's, so sizes that disagree with the graph give wrong values, never a fault.
 * RELGNN_EINVAL: first < 0, first >= last, last > V, a slice outside [0, M], a negative length, a null pointer where something is
 *   read or written, an edge array that is not 8-byte aligned.  RELGNN_EUNSUPPORTED: V < 1, L < 1 or V * L >= 2^31.  RELGNN_ENOSPC: a
 *   workspace smaller than relgnn_window_block_workspace_bytes(T, L).
 */
#ifndef RELGNN_WINDOW_BLOCK_H_
#define RELGNN_WINDOW_BLOCK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int relgnn_window_block_supported(int64_t num_nodes, int32_t num_edge_types);
/* the entries of one tile of the two flat passes (1024) */
int64_t relgnn_window_block_tile(void);
/* the storage of the scan over the T * L + 1 counts */
size_t relgnn_window_block_workspace_bytes(int64_t num_targets, int32_t num_edge_types);

int relgnn_window_block_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                              int64_t num_messages, int64_t first, int64_t last, int64_t entry_base, int64_t num_entries,
                              int32_t* stamp, int32_t* counts, int32_t* offsets, int32_t* totals, void* workspace,
                              size_t workspace_bytes, void* stream);

int relgnn_window_block_emit(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                             int64_t num_messages, int64_t first, int64_t last, int64_t entry_base, int64_t num_entries,
                             const int32_t* counts, const int32_t* offsets, const int32_t* outside, int64_t num_outside,
                             int32_t* stamp, int32_t* nodes, int64_t nodes_len, int32_t* edges, int64_t edges_len, float* degrees,
                             int64_t degrees_len, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_WINDOW_BLOCK_H_ */
