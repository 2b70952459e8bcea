/*
 * relgnn_subgraph.h — C ABI of librelgnn.so, subgraph sampling (the citation task's opt-in `subgraph_batches` mode): a node set
 * found by random walks over the by-target bucketing a RelGraph already holds, and the node-INDUCED subgraph over it: every edge of
 * the full graph whose two ends are in the set.  Every layer of a model runs on that one subgraph, whatever its depth.
 *
 * Declared beside relgnn_sampling.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller unless
 * it is marked HOST, `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.  No entry point synchronises; the caller reads the
 * subgraph's sizes back ONCE (tasks/subgraph_sampling.py), between induced_count and induced_emit.
 *
 * The graph: rowptr_t int32 [V * L + 1] over the rows `target * L + type`, col_t int32 [M] = `source * L + type`, the entries of
 *   a bucket in original message order (RelGraph.rowptr_t / col_t), read in place.
 *
 * The walk rule.  Walk w of R starts at roots[w] and takes h steps AGAINST the edges (a node's state depends on its in-neighbours).
 *   At node v the incoming entries of all types are one contiguous run of col_t, [b, e) = [rowptr_t[v * L], rowptr_t[(v + 1) * L]):
 *   the buckets (v, 0) .. (v, L - 1) are adjacent.  With deg = e - b, in step s = 0 .. h - 1:
 *     deg == 0  : the walk stays at v;
 *     otherwise : the next node is col_t[b + j] / L with j = (word * deg) >> 32 (the high half of the 32 x 32 -> 64 bit product),
 *                 word = output word 0 of Philox4x32-10 with counter = (w, s, draw, 0), key = (seed, replica).
 *   `draw` is the 32-bit count of sampled batches so far.  Every visited node, the roots included, is stamped 1 in `stamp`
 *   (int32 [V], all zero between calls) with plain stores, every writer writing the same value.  The node set is a pure function
 *   of (seed, replica, draw, the root list, h): the same set on every run, on any stream, whatever the launch shape.  A walk that
 *   meets a self loop or a dead end revisits: the set holds at most min(V, R * (h + 1)) nodes.
 *
 * The induced subgraph of a stamped node set (stamp[v] != 0; the walks' set, or any set the caller stamped with
 *   relgnn_neighbour_sample_begin).  `nodes` = the stamped nodes ascending (relgnn_neighbour_sample_compact with value 0: the
 *   flag scan is not forked); local id = position in `nodes`.  Of every bucket (t, l) with t in the set, the entries whose source is
 *   in the set are kept, in the bucket's own order.  Per type the kept edges of all targets, targets ascending, are the type's list
 *   {local(source), local(target)}; the types' lists lie one behind the other in ONE edge buffer.  degrees[l * n + i] = the number
 *   of kept entries of bucket (nodes[i], l): the INDUCED in-degree.
 *
 * Order of calls for one subgraph (B = node_bound >= the set's size; sizes are HOST values unless they are pointers):
 *     walk                        (or relgnn_neighbour_sample_begin over a given node list)
 *     relgnn_neighbour_sample_compact(stamp, V, 0, nodes, B, node_count, ...)
 *     number                      stamp[nodes[i]] = i + 1: a source's local id is then one load
 *     induced_count               counts / offsets / totals, layout as a hop's in relgnn_sampling.h:
 *                                   counts  int32 [L * B + 1] TYPE-MAJOR, counts[l * B + i] = kept entries of bucket (nodes[i], l),
 *                                           0 for i beyond the set and in the closing entry
 *                                   offsets int32 [L * B + 1] the exclusive prefix sums of counts (rocPRIM's device scan)
 *                                   totals  int32 [L + 1]     edges per type, then the edge total (from the offsets)
 *     -- the caller reads n = *node_count and totals back: the one read-back --
 *     induced_emit                edges int32 [edge_bound][2] (edge_bound >= the edge total; nothing is written at or beyond it),
 *                                 degrees float32 [L, n]
 *     clear                       stamp[nodes[i]] = 0, i in [0, n)
 *
 * Supported (relgnn_subgraph_supported; RELGNN_EUNSUPPORTED otherwise): 1 <= R, 0 <= h <= 64, V * L < 2^31.  h == 0 is legal: the
 *   subgraph induced on the roots alone.
 * The kernels TRUST the graph structure (monotone rowptr_t, 0 <= col_t < V * L) and the root list (in range): the caller validates
 *   both on the host.  A kernel fault is never the error path.
 * Kernels: every loop is bounded by a bucket length or a launch argument; no spin-wait, no hand-over between workgroups, no atomics.
 *   One lane owns one walk.  One WAVE owns one (subgraph node, type) bucket of any length: the lanes stride over it 64 entries at a
 *   pass, and a kept entry's slot is the bucket's offset + the kept entries of the earlier passes + the number of kept entries in
 *   lower lanes (popcount of the ballot).  A long bucket is not split over a workgroup.
 */
#ifndef RELGNN_SUBGRAPH_H_
#define RELGNN_SUBGRAPH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if (R = num_walks, h = walk_length, V = num_nodes, L = num_edge_types) is taken, else 0 */
int relgnn_subgraph_supported(int64_t num_walks, int32_t walk_length, int64_t num_nodes, int32_t num_edge_types);
/* the largest walk length (64) */
int64_t relgnn_subgraph_max_walk_length(void);
/* bytes of workspace for induced_count (max_items = L * B + 1) */
size_t relgnn_subgraph_workspace_bytes(int64_t max_items);

int relgnn_subgraph_walk(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                         const int32_t* roots, int64_t num_walks, int32_t walk_length, uint32_t draw, uint32_t seed,
                         uint32_t replica, int32_t* stamp, void* stream);

/* stamp[nodes[i]] = i + 1, i in [0, min(*node_count, node_bound)) */
int relgnn_subgraph_number(const int32_t* nodes, const int32_t* node_count, int64_t node_bound, int32_t* stamp, int64_t num_nodes,
                           void* stream);

int relgnn_subgraph_induced_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                  const int32_t* nodes, const int32_t* node_count, int64_t node_bound, const int32_t* stamp,
                                  int32_t* counts, int32_t* offsets, int32_t* totals, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* n = the set's size, a HOST value here (n <= node_bound); `stamp` as relgnn_subgraph_number left it */
int relgnn_subgraph_induced_emit(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                 const int32_t* nodes, int64_t n, int64_t node_bound, const int32_t* stamp, const int32_t* offsets,
                                 int64_t edge_bound, int32_t* edges, float* degrees, void* stream);

/* stamp[nodes[i]] = 0, i in [0, n) */
int relgnn_subgraph_clear(const int32_t* nodes, int64_t n, int32_t* stamp, int64_t num_nodes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SUBGRAPH_H_ */
