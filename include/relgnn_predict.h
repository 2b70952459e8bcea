/*
 * relgnn_predict.h — C ABI of librelgnn.so, predictions out of the task heads' logits.
 *
 * Declared beside relgnn.h, whose conventions hold here too: every pointer is a DEVICE pointer owned by the caller,
 * `stream` is a hipStream_t passed as void*, all work is enqueued asynchronously, every entry point returns an int
 * status (RELGNN_OK == 0) and never throws, nothing is allocated or retained, there is no global state.
 *
 * What a prediction is follows the reference's metric code to the bit, and each rule has ONE definition in the library
 * (csrc/common.h), called by the metric kernel that counts the label and by the kernel here that writes it:
 *     sigmoid_label     relgnn_sigmoid_ce_stats   (relgnn.h)   and relgnn_predict_sigmoid_f32
 *     row_lse           relgnn_softmax_ce_stats   (relgnn.h)   and relgnn_predict_softmax_f32
 *     candidate_choice  relgnn_varmisuse_head_fwd (relgnn.h)   and relgnn_predict_candidates_f32
 *
 * rows == 0 launches nothing and returns RELGNN_OK.  Outputs are written at caller-given leading dimensions (in
 * elements), so they may be slices of one packed arena; rows of a matrix must not overlap.  No workspace, no atomics.
 *
 * Compiled for gfx950 (registers / scratch bytes per kernel, from the code object's metadata):
 *     predict_sigmoid_kernel     <vector, packed labels> 35 VGPR / 0,  <vector> 29 / 0,  <scalar> 23 / 0
 *     predict_softmax_kernel     <1 lane per row> 31 / 0,  <16 lanes> 49 / 0,  <64 lanes> 51 / 0
 *     predict_candidates_kernel  36 / 0
 */
#ifndef RELGNN_PREDICT_H_
#define RELGNN_PREDICT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* PPI.  Replaces utils/utils.py:61-74 (reference file:line, relative to the reference root):
 *     predicted = tf.round(tf.nn.sigmoid(logits))
 * probs[r, c]  = sigmoid(logits[r, c]) in float32, in the form that cannot overflow:
 *                e = expf(-|x|);  1 / (1 + e) for x >= 0,  e / (1 + e) for x < 0.
 * labels[r, c] = 1 iff x > 0 and 1 / (1 + e) > 0.5 (round-half-even of the float32 sigmoid), else 0: the prediction
 *                whose true / false positives relgnn_sigmoid_ce_stats counts.  A logit of 1e-8 is a 0.
 * NaN -> probability NaN, label 0;  +inf -> 1, 1;  -inf -> 0, 0.
 * logits [rows, ld], probs [rows, ld_probs] float32 (4-byte aligned), labels [rows, ld_labels] uint8 (any address);
 * ld, ld_probs, ld_labels >= cols >= 1.  float4 / packed accesses where every pointer and leading dimension allows
 * (dense rows, ld == ld_probs == ld_labels == cols, are walked as one long row), scalar accesses otherwise. */
int relgnn_predict_sigmoid_f32(const float* logits, int64_t ld, int64_t rows, int64_t cols, float* probs,
                               int64_t ld_probs, uint8_t* labels_u8, int64_t ld_labels, void* stream);

/* Citation networks.  Replaces tasks/citation_network_task.py:134-138:
 *     predicted = tf.argmax(logits, axis=1)         (probabilities: tf.nn.softmax(logits))
 * probs[r, c] = expf(x[r, c] - max_r) / sum_c expf(x[r, c] - max_r) in float32.  A -inf column has probability exactly
 *               0.  A row holding NaN or +inf, or nothing but -inf, is NaN throughout (as torch.softmax); its class is
 *               unspecified; no other row is touched.
 * classes[r]  = the lowest index of the row's maximum logit: comparisons only, relgnn_softmax_ce_stats' rule.
 * logits [rows, ld], probs [rows, ld_probs] float32, classes int32 [rows]; ld, ld_probs >= cols >= 1, any cols. */
int relgnn_predict_softmax_f32(const float* logits, int64_t ld, int64_t rows, int32_t cols, float* probs,
                               int64_t ld_probs, int32_t* classes_i32, void* stream);

/* VarMisuse.  Replaces tasks/varmisuse_task.py:438:
 *     predicted = tf.argmax(tf.nn.softmax(logits), axis=1)
 * m = max_c x[c] (first);  e[c] = expf(x[c] - m);  sum = 1 + (sum of the other e[c], in index order);  probs[c] =
 * e[c] / sum;  predicted = the lowest index of the largest PROBABILITY, which two logits one ulp apart can share: the
 * arithmetic and the choice of relgnn_varmisuse_head_fwd's num_correct_predictions.  A padded candidate (logit
 * -1e7) has probability exactly 0.
 * logits, probs float32 [rows, cols] dense, predicted int32 [rows]; 1 <= cols <= 8. */
int relgnn_predict_candidates_f32(const float* logits, int64_t rows, int32_t cols, float* probs,
                                  int32_t* predicted_i32, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RELGNN_PREDICT_H_ */
