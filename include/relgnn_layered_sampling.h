/*
 * relgnn_layered_sampling.h — C ABI of librelgnn.so, the hop-ordered numbering of a sampled subgraph (the citation task's opt-in
 * `sampled_batches` key "layered"; NeighbourSampler.sample_by_hop).  Declared beside relgnn_sampling.h, whose conventions, rule and
 * order of calls hold here ("The hop-ordered numbering" there): every pointer is a DEVICE pointer owned by the caller unless it is
 * marked HOST, `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int status
 * (RELGNN_OK == 0) and never throws, nothing is allocated or retained, nothing synchronises.
 *
 * The rule.  The hops, the Philox draws and the sampled edges are those of relgnn_sampling.h for the same (seed, replica, draw); only
 *   the local numbering differs.  `nodes` holds the seeds in ascending id, then the nodes first reached in hop 1 in ascending id, ...,
 *   then those first reached in hop H; local id = position.  With n_d the number of nodes at most d hops from a seed, the nodes first
 *   reached in hop d are the local range [n_{d-1}, n_d).  A node's hop is in the stamp array until finish clears it (seeds carry -1).
 *   The adjacency lists keep their layout (hops ascending, targets ascending inside a hop, positions ascending inside a target), so
 *   the edges whose target is at most d hops from a seed are a prefix of every type's list.
 * Kernels: every loop is bounded by a segment length (at most 32 halvings) or a count known before the launch; every id written lies
 *   in [0, n) and every store is checked against the n the host passed; no atomics, no LDS, no spin-wait.  They read the stamps and
 *   write none: the stamps are cleared by relgnn_neighbour_sample_finish, as ever.
 */
#ifndef RELGNN_LAYERED_SAMPLING_H_
#define RELGNN_LAYERED_SAMPLING_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the hop-ordered relabel: out[e] = {local(source), local(target)} of edges[first + e], e in [0, count), with
 * local(v) = hop_starts[d] + the rank of v in nodes[hop_starts[d] .. hop_starts[d + 1]) (ascending), d = the hop that first reached v
 * (stamp[v]; -1, a seed, counts as 0).  hop_starts HOST int64 [num_levels + 1], 0 = hop_starts[0] <= ... <= hop_starts[num_levels] = n,
 * 1 <= num_levels <= 9 (the hops + 1).  A d outside [0, num_levels) is clamped and every id written lies in [0, n): a stamp array that
 * does not belong to `nodes` gives wrong ids, never a store or a load out of bounds.  Must run before finish. */
int relgnn_neighbour_sample_relabel_by_hop(const int32_t* edges, int64_t first, int64_t count, const int32_t* stamp,
                                           int64_t num_nodes, const int32_t* nodes, const int64_t* hop_starts, int32_t num_levels,
                                           int32_t* out, void* stream);

/* degrees[l * n + base + i] = (float)counts[l * frontier_bound + i], i in [0, frontier_count): the frontier of a hop is the local
 * range [base, base + frontier_count) of the hop-ordered numbering; frontier_count, base and n are HOST values,
 * base + frontier_count <= n (RELGNN_EINVAL otherwise) */
int relgnn_neighbour_sample_degrees_by_hop(const int32_t* counts, int64_t frontier_bound, int64_t frontier_count,
                                           int32_t num_edge_types, int64_t base, int64_t n, float* degrees, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_LAYERED_SAMPLING_H_ */
