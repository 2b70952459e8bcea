/*
 * graph_partition.h — PACKAGE-INTERNAL entry points of librelgnn.so: the wish pass of the device graph partitioner
 * (tasks/graph_partition.py; DESIGN.md section 3 states the whole rule).  NOT part of the public C ABI: nothing under include/
 * declares these, tf_gnn_samples_amd/_lib.py binds them from its table INTERNAL, and they may change with the package.
 *
 * The conventions of include/relgnn_subgraph.h hold: every pointer is a DEVICE pointer owned by the caller, `stream` is a
 * hipStream_t passed as void* and the last argument, all work is enqueued asynchronously, every entry point returns an int status
 * (RELGNN_OK == 0) and never throws, nothing is allocated or retained, nothing synchronises.
 *
 * The graph: rowptr_t int32 [V * L + 1], col_t int32 [M] = `source * L + type` (RelGraph.rowptr_t / col_t), read in place.  The
 *   in-neighbour multiset N(v) is col_t[j] / L over j in [rowptr_t[v * L], rowptr_t[(v + 1) * L]): the buckets of all types are one
 *   contiguous run (the walk rule of relgnn_subgraph.h), multiplicity counts, entries whose source is v itself are skipped.
 *
 * One wish pass.  part int32 [V] (-1: unassigned), room int32 [P], both of the round's start.  For an ELIGIBLE node v, with
 *   c(l) = |{u in N(v): part[u] == l}| (unassigned neighbours count nowhere) and base = c(part[v]) (0 for an unassigned v):
 *     wish[v] = the lowest l among those that maximise c(l) over the labels with l != part[v], room[l] > 0 and c(l) > base;
 *     wish[v] = -1 when there is none, and for every node that is not eligible.
 *   Eligible: refine == 0 (grow): part[v] < 0.
 *             refine != 0: anchor[v] == 0 and (Philox4x32-10(counter = (v, round, 0, 0), key = (seed, 0x10000000)).x & 1) == 1
 *             (csrc/philox.h; anchor int32 [V], non-zero for the nodes that never move).
 *   wish[v] is written for every v the selected row classes cover, a pure function of the arguments: the same on any stream, in
 *   any run, whatever the launch shape.
 *
 * Row classes (`classes`, a bit mask; 3 for a whole pass, the single bits for measurements):
 *   1  rows of at most relgnn_partition_wave_row_max() = 64 entries: one WAVE per node, one entry per lane, the labels counted by a
 *      ballot match loop of at most 64 turns;
 *   2  longer rows, listed by the caller: long_nodes int32 [long_bound] ascending, *long_count of them (a DEVICE count, clamped to
 *      long_bound; a list that names a short row is served all the same).  One WORKGROUP per node: a count table of P int32 in
 *      LDS (at most 32 KB), the lanes of all its waves stride over the row, integer LDS adds, a workgroup arg-max.
 *   No global atomics, no float atomics, no spin-wait, no hand-over between workgroups; every loop is bounded by a row length, P or
 *   a launch argument.
 *
 * Supported (relgnn_partition_supported; RELGNN_EUNSUPPORTED otherwise): V >= 1, L >= 1, V * L < 2^31, 1 <= P <= min(V, 8192),
 *   0 <= imbalance_percent <= 100, 0 <= refine_rounds <= 64.
 * The kernels TRUST the graph structure (monotone rowptr_t, 0 <= col_t < V * L), validated on the host as elsewhere; a label
 *   outside [0, P) counts as unassigned.  A kernel fault is never the error path.  num_nodes == 0 is RELGNN_OK and no launch.
 */
#ifndef RELGNN_GRAPH_PARTITION_H_
#define RELGNN_GRAPH_PARTITION_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if the partitioner takes (V, L, P, b, T), else 0 */
int relgnn_partition_supported(int64_t num_nodes, int32_t num_edge_types, int64_t num_parts, int32_t imbalance_percent,
                               int32_t refine_rounds);
/* the longest row of class 1 (64) */
int64_t relgnn_partition_wave_row_max(void);

int relgnn_partition_wish(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                          int64_t num_messages, const int32_t* part, const int32_t* room, int32_t num_parts, const int32_t* anchor,
                          int32_t refine, uint32_t round, uint32_t seed, const int32_t* long_nodes, const int32_t* long_count,
                          int64_t long_bound, int32_t classes, int32_t* wish, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_GRAPH_PARTITION_H_ */
