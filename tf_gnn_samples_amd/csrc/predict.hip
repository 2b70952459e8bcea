// Predictions out of the task heads' logits (include/relgnn_predict.h): probabilities and the label / class / candidate that the
// metric kernels count, decided by the SAME device functions (common.h: sigmoid_label, row_lse, candidate_choice).
//   PPI        utils/utils.py:61-74                    sigmoid, round(sigmoid) -> uint8 labels
//   Citation   tasks/citation_network_task.py:134-138  row softmax, tf.argmax of the logits
//   VarMisuse  tasks/varmisuse_task.py:438             tf.argmax(tf.nn.softmax(logits)) over <= 8 candidates
// Three elementwise / row-wise kernels over a few MB at most: bandwidth-trivial beside the forward pass that made the logits, not
// tuned.  No atomics, no workspace, no global state; every store is a plain or vector store.
#include "common.h"
#include "../../include/relgnn_predict.h"

using namespace relgnn;

namespace {

// ---- PPI ------------------------------------------------------------------------------------------------------------------------
// p = 1 / (1 + e) for x >= 0, e / (1 + e) for x < 0, e = expf(-|x|): no overflow, sigmoid(-inf) = 0, sigmoid(+inf) = 1, NaN -> NaN.
// For x > 0 the quotient is the one sigmoid_label compares with 0.5.
__device__ __forceinline__ void sigmoid_element(float x, float& p, uint8_t& l) {
  const float e = expf(-fabsf(x));
  const float d = 1.f + e;
  p = x >= 0.f ? 1.f / d : e / d;
  l = sigmoid_label(x, e) ? 1 : 0;
}

// One thread owns four consecutive columns of one row per grid pass.  VEC: float4 load / store of a whole group (the host has checked
// the pointers and leading dimensions); VECL: the four labels as one 32-bit store.  Scalar accesses otherwise and for a row's tail.
template <bool VEC, bool VECL>
__global__ __launch_bounds__(256) void predict_sigmoid_kernel(const float* __restrict__ X, long long ld, long long rows, long long cols,
                                                              float* __restrict__ P, long long ldp, uint8_t* __restrict__ L,
                                                              long long ldl) {
  const long long per_row = (cols + 3) >> 2, total = rows * per_row;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    const long long r = j / per_row, c = (j - r * per_row) << 2;
    const float* x = X + r * ld + c;
    float* p = P + r * ldp + c;
    uint8_t* l = L + r * ldl + c;
    if (VEC && c + 4 <= cols) {
      const float4 v = *reinterpret_cast<const float4*>(x);
      float4 o;
      uint8_t b0, b1, b2, b3;
      sigmoid_element(v.x, o.x, b0);
      sigmoid_element(v.y, o.y, b1);
      sigmoid_element(v.z, o.z, b2);
      sigmoid_element(v.w, o.w, b3);
      *reinterpret_cast<float4*>(p) = o;
      if (VECL) {
        *reinterpret_cast<uchar4*>(l) = make_uchar4(b0, b1, b2, b3);
      } else {
        l[0] = b0; l[1] = b1; l[2] = b2; l[3] = b3;
      }
    } else {
      for (int e = 0; e < 4 && c + e < cols; ++e) sigmoid_element(x[e], p[e], l[e]);
    }
  }
}

// ---- Citation ---------------------------------------------------------------------------------------------------------------------
// The stats kernel's row groups (W lanes per row).  The class is row_lse's idx; the probabilities are exp(x - m) / sum with the sum
// of all cols exponentials (a lane's share in column order, the W shares by a butterfly): a NaN or +inf column makes the sum, and
// so the whole row, NaN, as torch.softmax does (row_lse's own t leaves such columns out); an all -inf row is exp(NaN) throughout.
template <int W>
__global__ __launch_bounds__(256) void predict_softmax_kernel(const float* __restrict__ logits, long long ld, long long rows, int cols,
                                                              float* __restrict__ probs, long long ldp, int* __restrict__ classes) {
  constexpr int kRowsPerBlock = 256 / W;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  for (long long base = (long long)blockIdx.x * kRowsPerBlock; base < rows; base += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = base + g;
    const bool valid = r < rows;                     // (every lane of a wave runs the butterflies; a lane past the last row walks nothing)
    const float* row = logits + (valid ? r : 0) * ld;
    const int n = valid ? cols : 0;
    const RowLse a = row_lse<W>(row, n, j);
    float s = 0.f;
    for (int c = j; c < n; c += W) s += expf(row[c] - a.m);
#pragma unroll
    for (int off = W >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (!valid) continue;
    float* out = probs + r * ldp;
    for (int c = j; c < n; c += W) out[c] = expf(row[c] - a.m) / s;
    if (j == 0) classes[r] = a.idx;
  }
}

// ---- VarMisuse --------------------------------------------------------------------------------------------------------------------
// one thread per row of <= 8 logits
__global__ __launch_bounds__(256) void predict_candidates_kernel(const float* __restrict__ logits, long long rows, int cols,
                                                                 float* __restrict__ probs, int* __restrict__ predicted) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
    float x[kMaxCandidates], p[kMaxCandidates];
#pragma unroll
    for (int c = 0; c < kMaxCandidates; ++c) x[c] = c < cols ? logits[r * cols + c] : 0.f;
    const CandidateChoice ch = candidate_choice(x, cols, p);
#pragma unroll
    for (int c = 0; c < kMaxCandidates; ++c)
      if (c < cols) probs[r * cols + c] = p[c];
    predicted[r] = ch.arg;
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int relgnn_predict_sigmoid_f32(const float* logits, int64_t ld, int64_t rows, int64_t cols, float* probs, int64_t ld_probs,
                               uint8_t* labels_u8, int64_t ld_labels, void* stream) {
  if (rows < 0 || cols < 1 || ld < cols || ld_probs < cols || ld_labels < cols) return RELGNN_EINVAL;
  if (rows == 0) return RELGNN_OK;
  if (!logits || !probs || !labels_u8) return RELGNN_EINVAL;
  if (rows > INT64_MAX / ((cols + 3) >> 2)) return RELGNN_EINVAL;
  if (ld == cols && ld_probs == cols && ld_labels == cols) {      // dense rows: one long row, so that cols = 121 takes the vector path
    if (rows > INT64_MAX / cols) return RELGNN_EINVAL;
    cols *= rows;
    rows = 1;
    ld = ld_probs = ld_labels = cols;
  }
  const bool vec = aligned16(logits) && aligned16(probs) && (rows == 1 || ((ld & 3) == 0 && (ld_probs & 3) == 0));
  const bool vecl = vec && aligned4(labels_u8) && (rows == 1 || (ld_labels & 3) == 0);
  const unsigned grid = flat_grid(rows * ((cols + 3) >> 2), 256);
  hipStream_t s = as_stream(stream);
  if (vecl) predict_sigmoid_kernel<true, true><<<grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, labels_u8, ld_labels);
  else if (vec) predict_sigmoid_kernel<true, false><<<grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, labels_u8, ld_labels);
  else predict_sigmoid_kernel<false, false><<<grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, labels_u8, ld_labels);
  return launch_status();
}

int relgnn_predict_softmax_f32(const float* logits, int64_t ld, int64_t rows, int32_t cols, float* probs, int64_t ld_probs,
                               int32_t* classes_i32, void* stream) {
  if (rows < 0 || cols < 1 || ld < cols || ld_probs < cols) return RELGNN_EINVAL;
  if (rows == 0) return RELGNN_OK;
  if (!logits || !probs || !classes_i32) return RELGNN_EINVAL;
  const int w = softmax_group_width(cols);
  const long long per_block = 256 / w;
  long long grid = (rows + per_block - 1) / per_block;
  if (grid > 256 * 8) grid = 256 * 8;
  hipStream_t s = as_stream(stream);
  if (w == 1) predict_softmax_kernel<1><<<(unsigned)grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, classes_i32);
  else if (w == 16) predict_softmax_kernel<16><<<(unsigned)grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, classes_i32);
  else predict_softmax_kernel<64><<<(unsigned)grid, 256, 0, s>>>(logits, ld, rows, cols, probs, ld_probs, classes_i32);
  return launch_status();
}

int relgnn_predict_candidates_f32(const float* logits, int64_t rows, int32_t cols, float* probs, int32_t* predicted_i32, void* stream) {
  if (rows < 0 || cols < 1 || cols > kMaxCandidates) return RELGNN_EINVAL;
  if (rows == 0) return RELGNN_OK;
  if (!logits || !probs || !predicted_i32) return RELGNN_EINVAL;
  predict_candidates_kernel<<<flat_grid(rows, 256), 256, 0, as_stream(stream)>>>(logits, rows, cols, probs, predicted_i32);
  return launch_status();
}

}  // extern "C"
