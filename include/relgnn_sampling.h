/*
 * relgnn_sampling.h — C ABI of librelgnn.so, neighbour sampling (the citation task's opt-in `sampled_batches` mode): a
 * fanout-limited neighbourhood of a seed list, drawn on the device from the by-target bucketing a RelGraph already holds, and
 * the relabelled subgraph of it.
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller unless it is
 * marked HOST, `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.  No entry point synchronises; the caller decides
 * where a count is read back (tasks/neighbour_sampling.py: once per call when every fanout is positive, once more per hop whose
 * fanout is 0).
 *
 * The graph: rowptr_t int32 [V * L + 1] over the rows `target * L + type`, col_t int32 [M] = `source * L + type`, the entries of
 *   a bucket in original message order (RelGraph.rowptr_t / col_t).  It is read in place; no second copy of it is made.
 *
 * The rule.  Hops run h = 0 .. H - 1.  The frontier of hop 0 is the seed list in ascending node id.  For every frontier node t and
 *   edge type l, with deg the length of bucket t * L + l and k = fanouts[h]:
 *     k == 0 or deg <= k : every entry of the bucket is taken;
 *     otherwise          : exactly k entries, those with the smallest (word_j, j) in lexicographic order, where word_j is output
 *                          word j % 4 of Philox4x32-10 with
 *                              counter = (j / 4, t * L + l, h, draw),   key = (seed, 0x80000000 | replica).
 *                          (The dropout kernels' second key word is the small replica number: no dropout draw uses this key.)
 *   `draw` is the 32-bit count of sampled batches so far.  Taken entries are emitted in ascending j: the summation order of the
 *   bucket survives.  The sample is a pure function of (seed, replica, draw, hop, target, type, position): the same bits on every
 *   run, on any stream, whatever the launch shape.  Every entry of a bucket has the same chance k / deg.
 *   Every source of a taken entry that is not yet in the subgraph is stamped with h + 1 in `stamp` (int32 [V], all zero between
 *   calls; seeds carry -1) with plain stores, every writer of a hop writing the same value.  The frontier of hop h + 1 is the nodes
 *   stamped h + 1 in ascending id: every node is expanded at most once, and the nodes first reached in the last hop are leaves
 *   without an incoming edge (not even their self loop).
 *   Local ids are the ascending global ids of all stamped nodes, seeds included.
 *
 * Order of calls for one sample (all sizes the caller passes are HOST values; `*_bound` are capacities, the true counts live on
 * the device until the caller reads `totals` back):
 *     begin                                     seeds -> stamp = -1
 *     per hop:  count, take, compact(h + 1)     (count fills counts / offsets / totals; take emits and stamps; compact gives the
 *                                                next frontier and its length)
 *     compact(0)                                all stamped nodes, ascending: the subgraph's `nodes`
 *     per hop and type: relabel;  per hop: degrees;  finish (seed mask, stamps of the n visited nodes back to 0)
 *
 * The hop-ordered numbering (NeighbourSampler.sample_by_hop; the citation task's `"layered": true`).  The same hops, draws and
 *   edges; only the local ids differ.  `nodes` is the seed list, then the frontier of hop 1, ..., then the nodes first reached in
 *   hop H (the list compact(H) gives), each segment in ascending id; local id = position.  With n_d the number of nodes at most d hops
 *   from a seed, the nodes first reached in hop d are the local range [n_{d-1}, n_d), and because hops come out ascending inside every
 *   type's list, the edges whose target is below n_d are a prefix of that list.  Order of calls: as above through the last hop's
 *   compact(H); no compact(0); `nodes` is the concatenation of the frontier buffers cut to their true lengths (the caller's one
 *   read-back holds them); per hop and type relabel_by_hop, per hop degrees_by_hop, while the stamps still hold every node's hop;
 *   then finish over the hop-ordered `nodes` (it does not ask for an order), which clears the stamps and gives ones on [0, n_0).
 *   The two entry points are declared in relgnn_layered_sampling.h.
 *
 * Layout of a hop's arrays, with B = frontier_bound (>= the frontier's true length, which the kernels read from
 *   `frontier_count` on the device and clamp to B):
 *     counts  int32 [L * B + 1]  TYPE-MAJOR: counts[l * B + i] = min(deg, k) (deg where k == 0) of frontier node i and type l,
 *                                0 for i beyond the frontier; counts[L * B] = 0
 *     offsets int32 [L * B + 1]  the exclusive prefix sums of counts: the edges of type l lie in [offsets[l * B], offsets[(l + 1) * B])
 *                                of the hop's edge buffer, targets ascending, positions ascending inside a target
 *     totals  int32 [L + 1]      edges per type of this hop, then the hop's edge total
 *     edges   int32 [edge_bound][2] = {source, target} in GLOBAL ids; an entry at or beyond edge_bound is not written
 *   edge_bound >= the hop's edge total: min(B * L * k, M) when k > 0; with k == 0 the caller reads the total back first.
 *
 * Supported (relgnn_neighbour_sample_supported; RELGNN_EUNSUPPORTED otherwise): 1 <= H <= 8, 0 <= k <= 64, V * L < 2^31.
 * The kernels TRUST the graph structure (monotone rowptr_t, 0 <= col_t < V * L) and the seed list (in range, distinct, ascending):
 *   the caller validates both on the host.  A kernel fault is never the error path.
 * Kernels: every loop is bounded by a bucket length or a count known before the launch; no spin-wait, no hand-over between
 *   workgroups, no atomics.  One wave owns one (frontier node, type) bucket: lane q looks at positions q, q + 64, ... and keeps its
 *   smallest keys not yet taken; k rounds of a wave-wide arg-min take the k smallest whatever the bucket's length.
 */
#ifndef RELGNN_SAMPLING_H_
#define RELGNN_SAMPLING_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if (fanouts HOST int32 [num_hops], V = num_nodes, L = num_edge_types) is taken, else 0 */
int relgnn_neighbour_sample_supported(const int32_t* fanouts, int32_t num_hops, int64_t num_nodes, int32_t num_edge_types);
/* the largest fanout (64) and the largest number of hops (8) */
int64_t relgnn_neighbour_sample_max_fanout(void);
int64_t relgnn_neighbour_sample_max_hops(void);
/* bytes of workspace for count (max_items = L * B + 1) and compact (max_items = V) */
size_t relgnn_neighbour_sample_workspace_bytes(int64_t max_items);

/* stamp[seeds[i]] = -1 */
int relgnn_neighbour_sample_begin(const int32_t* seeds, int64_t num_seeds, int32_t* stamp, int64_t num_nodes, void* stream);

int relgnn_neighbour_sample_count(const int32_t* rowptr_t, int64_t num_nodes, int32_t num_edge_types, const int32_t* frontier,
                                  const int32_t* frontier_count, int64_t frontier_bound, int32_t fanout, int32_t* counts,
                                  int32_t* offsets, int32_t* totals, void* workspace, size_t workspace_bytes, void* stream);

int relgnn_neighbour_sample_take(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                 const int32_t* frontier, const int32_t* frontier_count, int64_t frontier_bound, int32_t fanout,
                                 int32_t hop, uint32_t draw, uint32_t seed, uint32_t replica, const int32_t* offsets,
                                 int64_t edge_bound, int32_t* stamp, int32_t* edges, void* stream);

/* out[0 .. *count) = the nodes v with stamp[v] == value (value != 0) or stamp[v] != 0 (value == 0), ascending; *count is clamped to
 * out_capacity and nothing is written beyond it */
int relgnn_neighbour_sample_compact(const int32_t* stamp, int64_t num_nodes, int32_t value, int32_t* out, int64_t out_capacity,
                                    int32_t* count, void* workspace, size_t workspace_bytes, void* stream);

/* out[e] = {local(source), local(target)} of edges[first + e], e in [0, count): local(v) = the position of v in nodes (ascending, n entries) */
int relgnn_neighbour_sample_relabel(const int32_t* edges, int64_t first, int64_t count, const int32_t* nodes, int64_t n,
                                    int32_t* out, void* stream);

/* degrees[l * n + local(frontier[i])] = (float)counts[l * frontier_bound + i], i in [0, frontier_count): frontier_count is a HOST value here */
int relgnn_neighbour_sample_degrees(const int32_t* counts, int64_t frontier_bound, int64_t frontier_count, int32_t num_edge_types,
                                    const int32_t* frontier, const int32_t* nodes, int64_t n, float* degrees, void* stream);

/* seed_mask[i] = (stamp[nodes[i]] == -1), then stamp[nodes[i]] = 0; `nodes` in any order */
int relgnn_neighbour_sample_finish(const int32_t* nodes, int64_t n, int32_t* stamp, int64_t num_nodes, float* seed_mask,
                                   void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SAMPLING_H_ */
