// THE element rule of TF1 Adam behind tf.clip_by_norm, shared by the dense multi-tensor launch (train_utils.hip:
// mt_adam_clip_kernel) and the row-deferred launches (sparse_update.hip).
#pragma once
#include "common.h"

namespace relgnn {

// gi = g * clip scale (formed by the caller), then
//   m = b1 m + (1-b1) gi;  v = b2 v + (1-b2) gi^2;  p -= lr_t * m / (sqrt(v) + eps)
// Every product and sum is rounded on its own (no contraction, whatever the compile flags say), so an element's new bits depend on
// its own (p, gi, m, v) and the scalars only — not on its position, the tensor's length, or which kernel ran it.  A row whose
// gradient is +0 is replayed by calling THIS function with gi = +0.f once per missed step: `m *= b1` is not the same rule
// (b1 * (-0) + (1-b1) * (+0) is +0, not -0).
__device__ __forceinline__ void adam_element(float& p, float gi, float& m, float& v, float lr_t, float b1, float b2, float eps) {
#pragma clang fp contract(off)
  const float mi = b1 * m + (1.f - b1) * gi;
  const float vi = b2 * v + (1.f - b2) * (gi * gi);
  m = mi;
  v = vi;
  p = p - lr_t * mi / (sqrtf(vi) + eps);
}

}  // namespace relgnn
