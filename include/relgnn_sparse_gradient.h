/*
 * relgnn_sparse_gradient.h — C ABI of librelgnn.so, the COMPACT gradient of a [F, n] row table whose gradient is +0
 * outside the rows a batch names (the weight of the sparse input projection under sampled batches, the citation task's
 * `"sparse_gradient": true`): which rows a batch names, the clip norm over those rows alone with the bits of the dense
 * norm, and the row-deferred Adam step (relgnn_sparse_update.h) reading a [T, n] gradient.
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * Replaces: nothing of the reference (dense Adam behind tf.clip_by_norm, models/sparse_graph_model.py:227-260).  What
 *           these entry points store and return are THE SAME BITS as relgnn_mt_l2norm and relgnn_rows_adam_step give
 *           for the dense [F, n] gradient that holds the compact rows and +0 everywhere else.
 *
 * ---- 1. Named rows ------------------------------------------------------------------------------------------------
 * rowptr_t int32 [F + 1] is the row pointer of a batch's transposed structure (relgnn_sparse_subset.h); word f is NAMED
 * when rowptr_t[f + 1] > rowptr_t[f].  With T named words:
 *   words     int32 [T]      the named words, ascending
 *   slot      int32 [F + 1]  the exclusive scan of the named flags: slot[words[t]] == t, slot[F] == T
 *   rowptr_c  int32 [T + 1]  rowptr_t without its repeats: rowptr_c[t] = rowptr_t[words[t]], rowptr_c[T] = rowptr_t[F]
 *   slabs_c [S][4], combos_c [C][3]  the transposed structure's long-row plan with every `row` field mapped through slot
 * (rowptr_c, the transposed structure's col and val as they are, slabs_c, combos_c and its ws_rows) is a CSR of T rows
 * that relgnn_csr_project_f32 takes unchanged; the summation order of a row depends on its length alone, so row t of
 * the [T, n] result has the bits of row words[t] of the [F, n] one.
 *   relgnn_named_rows_count  writes slot (a rocPRIM exclusive scan read through a transform iterator) and *count = T.
 *                            `count` may point into a buffer the caller reads back anyway.
 *   relgnn_named_rows_fill   writes words, rowptr_c, slabs_c and combos_c; T, num_slabs and num_combos are the
 *                            CAPACITIES of the outputs and every store is checked against them.  A plan row outside
 *                            [0, F) or without a slot below T (never, for a plan of the same structure) becomes an
 *                            empty entry of row 0.  T == 0 launches nothing.
 * No atomics, no spin-wait, no hand-over between workgroups; every loop is bounded by a launch argument.
 *
 * ---- 2. The norm: THE ORDER IS THE INTERFACE ------------------------------------------------------------------------
 * relgnn_mt_l2norm over a contiguous [F, n] gradient g sums in this order:
 *   a. element i = f * n + c belongs to slot i mod 8192 = block slot / 256, thread slot % 256;
 *   b. each slot adds double(g[i]) * double(g[i]) (exact) to +0.0 in ascending i;
 *   c. a 64-lane xor butterfly over offsets 32, 16, 8, 4, 2, 1;
 *   d. the four wave sums of a block combine as (r0 + r1) + (r2 + r3): 32 partials;
 *   e. one more butterfly over the 32 partials, padded with +0.0 to 64 lanes;
 *   f. (float)sqrt.
 * Adding +0.0 to a non-negative double changes nothing, so the result is a function of the named rows alone.
 * relgnn_rows_l2norm computes it from them: each slot sums, over t ascending, the one element (if any) of row t whose
 * (words[t] * n + c) mod 8192 is the slot (n <= 1024 < 8192: at most one c per row), then c. to f. as above
 * (csrc/norm_tree.h is the one definition both launches compile).  It writes the 32 doubles of d. to the front of
 * `workspace` and the float to norm[0].  T == 0: 32 times +0.0 and +0.0f.  A words[t] outside [0, F) is skipped.
 *   g float32 [T, n] with leading dimension ld_g >= n; n a multiple of 4 in 4 .. 1024 (relgnn_rows_adam_supported),
 *   whether or not it divides 8192.  Work distribution: 32 blocks; a block reads `words` in tiles, keeps — in order —
 *   the rows that meet its 256 slots, and each thread adds its element of those.  No atomics.
 *
 * ---- 3. The row step ------------------------------------------------------------------------------------------------
 * relgnn_rows_adam_step_compact is relgnn_rows_adam_step (relgnn_sparse_update.h: the replay of missed steps with
 * g = +0, the real step with g * scale, scale = clip > 0 ? clip / fmaxf(norm[0], clip) : 1, stamps[f] = t_new, one
 * store of step_sizes[t_new - base - 1] = lr_t) with the named rows given as words[T] and the gradient row of word
 * words[t] being g[t, :].  It walks words, 64 compact rows per wave, and never reads the other F - T rows' stamps.
 * `words` ascending and distinct (a word listed twice would be stepped twice).  The result does not depend on the grid
 * or the stream.  Shapes and alignment as relgnn_rows_adam_step; 0 <= T <= F.
 *
 * Anything outside the stated shapes is RELGNN_EINVAL / RELGNN_EUNSUPPORTED / RELGNN_ENOSPC before anything is
 * launched.  A kernel fault is never the error path.
 */
#ifndef RELGNN_SPARSE_GRADIENT_H_
#define RELGNN_SPARSE_GRADIENT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- named rows ---- */
size_t relgnn_named_rows_workspace_bytes(int64_t F);
int relgnn_named_rows_count(const int32_t* rowptr_t, int64_t F, int32_t* slot, int32_t* count, void* workspace,
                            size_t workspace_bytes, void* stream);
int relgnn_named_rows_fill(const int32_t* rowptr_t, int64_t F, const int32_t* slot, int64_t T, int32_t* words,
                           int32_t* rowptr_c, const int32_t* slabs_t, int32_t* slabs_c, int64_t num_slabs,
                           const int32_t* combos_t, int32_t* combos_c, int64_t num_combos, void* stream);

/* ---- the dense norm's bits over compact rows ---- */
size_t relgnn_rows_l2norm_workspace_bytes(void);
int relgnn_rows_l2norm(const int32_t* words, int64_t T, const float* g, int64_t ld_g, int32_t n, int64_t F, float* norm,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- the row step on compact rows ---- */
int relgnn_rows_adam_step_compact(const int32_t* words, int64_t T, int64_t F, float* p, const float* g, int64_t ld_g,
                                  float* m, float* v, int64_t ld, int32_t n, int32_t* stamps, float* step_sizes,
                                  int32_t base, int32_t t_new, const float* norm, float clip, float lr_t, float beta1,
                                  float beta2, float eps, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SPARSE_GRADIENT_H_ */
