/*
 * relgnn_dropout.h — C ABI of librelgnn.so, layer-input dropout (an opt-in route: RELGNN_LAYER_DROPOUT=fused).
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained.
 *
 * Replaces: tf.nn.dropout on every layer's input and the residual average behind it, models/sparse_graph_model.py:178-185
 *           (reference file:line, relative to the reference root):
 *               cur = tf.nn.dropout(cur, rate=1.0 - dropout_keep_prob)          # div(x, keep_prob) * mask
 *               if layer_idx % residual_every == 0:
 *                   t = cur;  if layer_idx > 0: cur += last;  cur /= 2;  last = t
 *
 * Random numbers: Philox4x32-10 (the Random123 constants), a pure function of the element:
 *     key     = (state[0] & 0xffffffff, state[1] & 0xffffffff)                      seed, replica
 *     counter = (g lo, g hi, stream_id, state[2] & 0xffffffff)                      g = (element_offset + i) / 4, step
 *     element i takes output word (element_offset + i) % 4;  keep iff (word >> 8) < T,  T = round(keep_prob * 2^24).
 *   `state` is int64[3] = {seed, replica, step} in DEVICE memory: the step is never a launch argument, so a captured
 *   launch draws the masks of whatever step the state holds when it runs.  No mask is stored; a backward call with
 *   the state block of its forward regenerates that forward's mask.
 *   element_offset must be a multiple of 4 (RELGNN_EINVAL otherwise); the package passes 0.  It places a small tensor
 *   anywhere in the 2^66-element counter space (the high counter word).
 * Arithmetic: a true fp32 division and a multiply by m in {0.0f, 1.0f}; a dropped +-inf or NaN is NaN, as in TF.
 * Contract: bit-exact against the composition written with each function, for any n >= 0 and any 4-byte aligned
 *           pointers (float4 accesses where every pointer is 16-byte aligned, scalar accesses otherwise).
 */
#ifndef RELGNN_DROPOUT_H_
#define RELGNN_DROPOUT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* y[i] = (x[i] / keep_prob) * m[i] */
int relgnn_dropout_fwd(const float* x, int64_t n, int64_t element_offset, const int64_t* state, int32_t stream_id,
                       uint32_t T, float keep_prob, float* y, void* stream);
/* gx[i] = (gy[i] / keep_prob) * m[i] */
int relgnn_dropout_bwd(const float* gy, int64_t n, int64_t element_offset, const int64_t* state, int32_t stream_id,
                       uint32_t T, float keep_prob, float* gx, void* stream);

/* residual layers after the first, one pass:  t[i] = (x[i] / keep_prob) * m[i];  cur[i] = (t[i] + last[i]) / 2 */
int relgnn_dropout_residual_fwd(const float* x, const float* last, int64_t n, int64_t element_offset,
                                const int64_t* state, int32_t stream_id, uint32_t T, float keep_prob, float* t,
                                float* cur, void* stream);
/* g_last[i] = g_cur[i] / 2;  g_x[i] = ((g_t[i] + g_cur[i] / 2) / keep_prob) * m[i]   (g_t may be NULL: no such term) */
int relgnn_dropout_residual_bwd(const float* g_t, const float* g_cur, int64_t n, int64_t element_offset,
                                const int64_t* state, int32_t stream_id, uint32_t T, float keep_prob, float* g_x,
                                float* g_last, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_DROPOUT_H_ */
