/*
 * level_plan.h — PACKAGE-INTERNAL entry points of librelgnn.so: the bucketings of the level graphs of a hop-ordered sampled batch,
 * DERIVED from the bucketing of its union graph instead of sorted again (tasks/neighbour_sampling.py, HopSubgraph.level_graphs;
 * DESIGN.md section 9).  NOT part of the public C ABI: nothing under include/ declares these, tf_gnn_samples_amd/_lib.py binds them
 * from its table INTERNAL, and they may change with the package.
 *
 * The conventions of include/relgnn_sampling.h hold: every pointer is a DEVICE pointer owned by the caller, `stream` is a hipStream_t
 * passed as void* and the last argument, all work is enqueued asynchronously, every entry point returns an int status
 * (RELGNN_OK == 0) and never throws, nothing is allocated or retained, nothing synchronises, nothing is read back.
 *
 * The union graph: V nodes numbered by hop, L edge types, M messages, with the eight arrays RelGraph computes for it (rowptr_t
 *   [V * L + 1], col_t / perm_t / inv_perm_t [M], rowptr_s [V * L + 1], tgt_s / frow_s / pos_t_of_s / perm_s [M]).
 * A level d (of num_levels <= relgnn_level_plan_max_levels() = 7 per call) is the graph over the first S_d nodes whose messages are
 *   the union's with a target below T_d; per edge type they are a PREFIX of the union's list, so the level's message m' of type l
 *   is the union's message m' + delta[l].  The level's arrays, every one what the stable sorts of RelGraph would give:
 *     rowptr_t' [S_d * L + 1] = rowptr_t[0 .. T_d * L], then P_d (the level's message count) behind it;
 *     perm_t'   [P_d]          = perm_t[p] - delta[col_t[p] % L];           (col_t' is col_t[0 .. P_d) itself: no copy is made)
 *     inv_perm_t' [P_d]        : inv_perm_t'[m'] = inv_perm_t[m' + delta[type of m']];
 *     tgt_s', frow_s', pos_t_of_s', perm_s' [P_d]: the STABLE compaction of the union's by-source entries q with tgt_s[q] < T_d;
 *                                tgt_s, frow_s and pos_t_of_s keep their values, perm_s'[.] = perm_s[q] - delta[frow_s[q] % L];
 *     rowptr_s' [S_d * L + 1]  : rowptr_s'[r] = the number of kept entries in front of rowptr_s[r].
 *
 * desc: int64 [num_levels * relgnn_level_plan_desc_stride(L)], one record per level:
 *     { T_d, S_d, P_d, then the offsets INTO `out` (in int32 elements) of rowptr_t', perm_t', inv_perm_t', rowptr_s', tgt_s',
 *       frow_s', pos_t_of_s', perm_s' (eight), then delta[0 .. L), then the level's type offsets off'[0 .. L] (off'[L] == P_d) }.
 *   The caller sizes `out` (int32 [out_len]) from the hop sizes it already holds; the regions must not overlap.
 * max_rows = the largest S_d * L + 1 and max_messages = the largest P_d over the levels size the launches.
 *
 * Shape of the work: the compaction is ONE flat pass over the M by-source entries for all levels (they are nested: one flag per
 *   level per entry).  Tiles of 1024 entries: per wave a ballot mask and its count per level, a scan of the 16 counts of a tile in
 *   LDS, the tile totals scanned by one workgroup, and a second flat pass that writes every kept entry to tile offset + wave offset
 *   + its rank in the mask.  The row pointers read the same masks.  The time is a function of M, V * L and num_levels, never of a
 *   bucket's length.  No atomics, no spin-wait, no hand-over between workgroups; the result is a pure function of the arguments on
 *   any stream.
 *
 * The kernels TRUST the union's arrays (they are RelGraph's own) but no index from `desc`: every store into `out` is checked against
 *   out_len and every load against its array's length, so a wrong record gives wrong values, never a fault.
 * RELGNN_EINVAL: a negative size, num_levels outside [0, 7], L < 1, V * L >= 2^31, max_rows > V * L + 1, max_messages > M, a null
 *   pointer where something is read or written, a workspace smaller than relgnn_level_plan_workspace_bytes.  num_levels == 0 is
 *   RELGNN_OK and no launch.
 */
#ifndef RELGNN_LEVEL_PLAN_H_
#define RELGNN_LEVEL_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most levels one call derives (7: a sampler of 8 hops has 7 levels below the union graph) */
int32_t relgnn_level_plan_max_levels(void);
/* int64 entries per level record of `desc`: 11 + 2 L + 1 */
int64_t relgnn_level_plan_desc_stride(int32_t num_edge_types);
/* the entries of one compaction tile (1024) */
int64_t relgnn_level_plan_tile(void);
size_t relgnn_level_plan_workspace_bytes(int64_t num_messages, int32_t num_levels);

int relgnn_level_plan(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, const int32_t* inv_perm_t,
                      const int32_t* rowptr_s, const int32_t* tgt_s, const int32_t* frow_s, const int32_t* pos_t_of_s,
                      const int32_t* perm_s, int64_t num_nodes, int32_t num_edge_types, int64_t num_messages, const int64_t* desc,
                      int32_t num_levels, int64_t max_rows, int64_t max_messages, int32_t* out, int64_t out_len, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_LEVEL_PLAN_H_ */
