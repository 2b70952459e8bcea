/*
 * relgnn_subgraph_norm.h — C ABI of librelgnn.so, GraphSAINT normalisation of subgraph batches (the key "normalisation" of the
 * citation task's `subgraph_batches`): visit counts over pre-sampled subgraphs, per-edge aggregation weights emitted with a batch's
 * induced edges, and a masked softmax cross-entropy head whose terms carry a per-row weight.
 *
 * Declared beside relgnn_subgraph.h, whose conventions and whose graph hold here too: every pointer is a DEVICE pointer owned by the
 * caller unless it is marked HOST, `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point
 * returns an int status (RELGNN_OK == 0) and never throws, nothing is allocated or retained, no entry point synchronises.
 *
 * The counts.  node_visits int32 [V] and edge_visits int32 [M], the latter aligned with col_t: after N pre-sampled subgraphs
 *   node_visits[v] = the number of them that hold v, edge_visits[p] = the number of them that hold BOTH ends of by-target entry p
 *   (the target of p's bucket and the source col_t[p] / L).  For a node-induced sampler that is GraphSAINT's C_v and C_{u,v}.
 *   Both arrays are all zero before the first launch; the caller zeroes them.
 *
 * Order of calls for one PRE-SAMPLED subgraph (relgnn_subgraph.h's, with the count in the place of induced_count .. emit):
 *     walk, relgnn_neighbour_sample_compact, number      as for a batch
 *     visit_count                 one wave per (subgraph node, type) bucket, the pass structure of induced_count: a kept entry at
 *                                 bucket offset j adds 1 to edge_visits[b + j] (b = rowptr_t[t * L + l]); the wave of type 0 adds 1
 *                                 to node_visits[t].  The set's size is read from the device pointer node_count, bounded by
 *                                 node_bound, as relgnn_subgraph_number reads it: NOTHING is read back by the host.
 *     -- the caller resets the stamp array (it zeroes it: the set's size never reaches the host) --
 *   One writer.  A node is in `nodes` once, so bucket (t, l) belongs to one wave of the launch, position b + j to one lane of that
 *   wave in one pass, and node_visits[t] to lane 0 of t's type-0 wave: every address has exactly one writer per launch, which loads,
 *   adds 1 and stores.  The launches of one stream are ordered.  So there are no atomics, and the counts are the same on every run.
 *   The caller keeps every launch that touches one pair of count arrays on ONE stream (or orders them by events).
 *
 * The weighted emit.  relgnn_subgraph_induced_emit_weighted writes what relgnn_subgraph_induced_emit writes — the same edges, the
 *   same induced in-degrees, bit for bit — and edge_weights float32 [edge_bound] in the order of `edges`.  For a kept entry at
 *   position p of bucket (t, l) whose full-graph length is deg = rowptr_t[t * L + l + 1] - rowptr_t[t * L + l]:
 *       a = (float)max(node_visits[t], 1) / (float)max(edge_visits[p], 1)
 *       a = fminf(a, max_edge_weight)
 *       edge_weights[slot] = a * (1.0f / ((float)deg + 1e-7f))
 *   The last factor is relgnn_degree_scale's expression over the FULL graph's in-degree of (t, l).  A sum aggregator over these
 *   weights estimates the full-graph aggregate sum_p X[col_t[p]] / (deg + 1e-7): over the pre-sampled subgraphs themselves,
 *   sum_b [p in b] * (C_t / C_p) / C_t == 1 for every entry that was seen and not clipped.
 *
 * The weighted loss head (beside relgnn_softmax_ce_stats / relgnn_softmax_ce_bwd of relgnn.h: the same row walk, the same double
 *   sums in a fixed order, the same ld / ldg conventions), with weights float32 [rows] and `denominator`, a HOST float:
 *       stats[0] = sum mask * weight * loss      stats[1] = sum mask      stats[2] = sum mask * [argmax == label]
 *       stats[3] = stats[0] / denominator        stats[4] = stats[2] / stats[1]      stats[5] = sum mask * weight
 *   [1], [2] and [4] are the UNWEIGHTED counts.
 *       glogits[v, c] = mask_v * weight_v * (softmax(logits_v)_c - [c == label_v]) * (g_total[0] + g_loss[0] / denominator)
 *   for c < cols, 0 for cols <= c < ldg; a row with mask 0 is zeros.  Either gradient pointer may be null, not both.  With every
 *   weight 1 and denominator == stats[1], stats[0 .. 4] and glogits are relgnn_softmax_ce_stats' and relgnn_softmax_ce_bwd's bits.
 *
 * Validated (RELGNN_EINVAL / RELGNN_EUNSUPPORTED / RELGNN_ENOSPC): sizes, bounds, null pointers, V * L < 2^31, M < 2^31, the
 *   alignment of `edges`, max_edge_weight > 0, denominator != 0 and not NaN.
 * TRUSTED, as in relgnn_subgraph.h: the graph structure (monotone rowptr_t with rowptr_t[V * L] == num_messages, 0 <= col_t < V * L)
 *   and that node_visits / edge_visits hold V / num_messages entries; labels outside [0, cols) cost no access.  A count launch
 *   nevertheless writes no position at or beyond num_messages, and a weighted emit reads none.
 * Kernels: every loop is bounded by a bucket length or a launch argument; no spin-wait, no hand-over between workgroups, no atomics.
 */
#ifndef RELGNN_SUBGRAPH_NORM_H_
#define RELGNN_SUBGRAPH_NORM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `stamp` as relgnn_subgraph_number left it; the set's size is min(*node_count, node_bound) */
int relgnn_subgraph_visit_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                int64_t num_messages, const int32_t* nodes, const int32_t* node_count, int64_t node_bound,
                                const int32_t* stamp, int32_t* node_visits, int32_t* edge_visits, void* stream);

/* relgnn_subgraph_induced_emit's arguments and results, and edge_weights float32 [edge_bound] */
int relgnn_subgraph_induced_emit_weighted(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                          int64_t num_messages, const int32_t* nodes, int64_t n, int64_t node_bound,
                                          const int32_t* stamp, const int32_t* offsets, const int32_t* node_visits,
                                          const int32_t* edge_visits, float max_edge_weight, int64_t edge_bound, int32_t* edges,
                                          float* degrees, float* edge_weights, void* stream);

/* bytes of workspace for relgnn_softmax_ce_weighted_stats */
size_t relgnn_softmax_ce_weighted_stats_workspace_bytes(void);

/* stats float32 [6] */
int relgnn_softmax_ce_weighted_stats(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                                     float denominator, int64_t rows, int32_t cols, float* stats, void* workspace,
                                     size_t workspace_bytes, void* stream);

int relgnn_softmax_ce_weighted_bwd(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                                   float denominator, int64_t rows, int32_t cols, const float* g_loss, const float* g_total,
                                   float* glogits, int64_t ldg, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SUBGRAPH_NORM_H_ */
