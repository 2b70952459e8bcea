/*
 * relgnn_sparse_update.h — C ABI of librelgnn.so, the row-deferred Adam update of a [F, n] row table whose gradient
 * is +0 outside the rows a batch names (the citation task's sampled batches over sparse node features: the weight of
 * the input projection, include/relgnn_sparse_features.h).
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * Replaces: nothing of the reference.  Its rule is dense Adam behind tf.clip_by_norm
 *           (models/sparse_graph_model.py:227-260), which relgnn_mt_adam_clip applies to every element every step.
 *           These entry points store THE SAME BITS while touching only the rows a step names.
 *
 * The scheme.  One step of dense Adam on an element whose (clipped) gradient is +0 is a pure function of
 * (p, m, v, lr_t).  A row that no entry of the batch's transposed structure names has such a gradient and is not read
 * by the projection's forward either, so it is left alone; `stamps[f]` says which step row f is current to, and the
 * steps it missed are replayed, with g = +0 and each step's own lr_t, before anything reads it again.  The replay
 * calls the element function of the dense launch (csrc/adam_element.h: products and sums rounded separately, f32
 * subnormals kept), once per missed step, so the stored bits are the dense launch's — a signed zero included, which
 * is why the replay is not `m *= beta1`.
 *
 * Shared arguments:
 *   rowptr_t    int32 [F + 1], the row pointer of the batch's transposed structure; row f is NAMED when
 *               rowptr_t[f + 1] > rowptr_t[f].  NULL: every row is named.
 *   p, m, v     float32 [F, n], leading dimension ld (in floats); g float32 [F, n], leading dimension ld_g.
 *   stamps      int32 [F]: row f holds the values dense Adam has after step stamps[f].
 *   step_sizes  float32: step_sizes[s - base - 1] is lr_t of step s, for base < s <= the newest step.  The caller
 *               keeps t - base within the table's length.
 *   base        no stamp is below it (the caller's duty; a stamp below base is read as base: the loop is clamped,
 *               nothing outside the table is read, the row's values are then not dense Adam's).
 *
 * relgnn_rows_adam_catch_up: every named row with stamps[f] < t_now replays steps stamps[f] + 1 .. t_now and gets
 *   stamps[f] = t_now.  A row that is current costs its stamp read.
 * relgnn_rows_adam_step: step t_new.  Every named row replays steps stamps[f] + 1 .. t_new - 1 if it is behind, then
 *   takes the real update with g[f, :] * scale and lr_t, scale = clip > 0 ? clip / fmaxf(norm[0], clip) : 1 exactly as
 *   relgnn_mt_adam_clip forms it (`norm`: this variable's entry of what relgnn_mt_l2norm wrote; may be NULL when
 *   clip <= 0), and gets stamps[f] = t_new.  One thread stores step_sizes[t_new - base - 1] = lr_t, the float the
 *   launch received.  Needs base < t_new.
 *
 * Work distribution: a wave reads the rowptr_t pairs and stamps of 64 consecutive rows, then walks the rows that
 *   have work one after the other, a lane holding 16 bytes of each array per pass.  No atomics, no LDS; the result
 *   does not depend on the grid or the stream.
 *
 * Shapes: n a multiple of 4 in 4 .. 1024 (relgnn_rows_adam_supported; RELGNN_EUNSUPPORTED otherwise); p, g, m, v
 *   16-byte aligned with leading dimensions that are multiples of 4 and >= n; 0 <= F < 2^31 - 1; 0 <= base <= t_now.
 *   Anything else is RELGNN_EINVAL.  A kernel fault is never the error path.
 */
#ifndef RELGNN_SPARSE_UPDATE_H_
#define RELGNN_SPARSE_UPDATE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 if rows of n floats are taken (n % 4 == 0, 4 <= n <= 1024), else 0 */
int relgnn_rows_adam_supported(int32_t n);

int relgnn_rows_adam_catch_up(const int32_t* rowptr_t, int64_t F, float* p, float* m, float* v, int64_t ld, int32_t n,
                              int32_t* stamps, const float* step_sizes, int32_t base, int32_t t_now, float beta1,
                              float beta2, float eps, void* stream);

int relgnn_rows_adam_step(const int32_t* rowptr_t, int64_t F, float* p, const float* g, int64_t ld_g, float* m, float* v,
                          int64_t ld, int32_t n, int32_t* stamps, float* step_sizes, int32_t base, int32_t t_new,
                          const float* norm, float clip, float lr_t, float beta1, float beta2, float eps, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_SPARSE_UPDATE_H_ */
