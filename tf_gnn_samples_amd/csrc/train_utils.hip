// Training-step plumbing AROUND the hot path, fused so that the step is not
// launch-bound once the gather/segment kernels and GEMMs are fast:
//   * multi-tensor per-variable clip_by_norm + TF-style Adam, RMSProp, SGD   models/sparse_graph_model.py:227-260
//   * PPI output head loss + micro-F1 counts in one pass        tasks/ppi_task.py:181-191, utils/utils.py:61-74
//   * citation head: masked softmax cross-entropy + accuracy     tasks/citation_network_task.py:133-148
// Deterministic (no float atomics): fixed-shape tree reductions only.
#include "common.h"
#include "adam_element.h"
#include "norm_tree.h"
#include "../../include/relgnn_subgraph_norm.h"
#include <type_traits>

using namespace relgnn;

namespace {

struct MtArgs {
  float* p[RELGNN_MT_MAX];
  const float* g[RELGNN_MT_MAX];
  float* m[RELGNN_MT_MAX];
  float* v[RELGNN_MT_MAX];
  long long n[RELGNN_MT_MAX];
};

struct NormArgs {
  const float* g[RELGNN_MT_MAX];
  long long n[RELGNN_MT_MAX];
};

__device__ __forceinline__ double block_sum_1024(double x, double* red) {
  // wave reduce (64 lanes) then across the 16 waves of a 1024-thread block, fixed order
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[wave] = x;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  __syncthreads();
  return t;  // valid in thread 0
}

// norms[t] = sqrt(sum g^2): grid (kNormChunks, tensors) of partial sums in double, then one small block per tensor
// adds the kNormChunks partials in a fixed order (deterministic; a single block per tensor took 35 us for the
// 196 k-element kernels of C2, this pair takes ~10 us).  The tree is norm_tree.h's, shared with sparse_gradient.hip.
__global__ __launch_bounds__(kNormBlock) void mt_l2norm_partial_kernel(NormArgs a, double* __restrict__ partial) {
  __shared__ double red[4];
  const int t = blockIdx.y;
  const float* g = a.g[t];
  const long long n = a.n[t];
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double x = g[i];
    acc += x * x;
  }
  const double sum = norm_block_partial(acc, red);
  if (threadIdx.x == 0) partial[(long long)t * kNormChunks + blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void mt_l2norm_final_kernel(const double* __restrict__ partial, float* __restrict__ norms) {
  const int t = blockIdx.x;
  const float norm = norm_of_partials(partial + (long long)t * kNormChunks);
  if (threadIdx.x == 0) norms[t] = norm;
}

// grid (chunks, tensors): g' = g * clip / max(||g||, clip)  (tf.clip_by_norm), then TF1 Adam:
//   m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr_t * m / (sqrt(v) + eps),  lr_t = lr sqrt(1-b2^t)/(1-b1^t)
// state[0] = number of Adam steps taken so far (as a float: exact up to 2^24), state[1] = lr_t of the step being taken.
// One thread: t += 1; lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t).  Keeps the step count ON THE DEVICE so that a captured
// hipGraph of the training step advances it on every replay (a host scalar would be frozen into the graph).
__global__ void adam_step_size_kernel(float* __restrict__ state, float lr, float b1, float b2) {
  const float t = state[0] + 1.f;
  state[0] = t;
  state[1] = lr * sqrtf(1.f - powf(b2, t)) / (1.f - powf(b1, t));
}

__global__ __launch_bounds__(256) void mt_adam_clip_kernel(MtArgs a, const float* __restrict__ norms, float clip,
                                                           float lr_t, const float* __restrict__ d_lr_t, float b1, float b2,
                                                           float eps) {
  if (d_lr_t) lr_t = d_lr_t[0];
  const int t = blockIdx.y;
  const long long n = a.n[t];
  const long long chunk = 4096;
  const long long beg = (long long)blockIdx.x * chunk;
  if (beg >= n) return;
  const long long end = min(n, beg + chunk);
  float scale = 1.f;
  if (clip > 0.f) {
    const float nrm = norms[t];
    scale = clip / fmaxf(nrm, clip);
  }
  float* p = a.p[t];
  const float* g = a.g[t];
  float* m = a.m[t];
  float* v = a.v[t];
  for (long long i = beg + threadIdx.x; i < end; i += blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_element(pi, g[i] * scale, mi, vi, lr_t, b1, b2, eps);      // (adam_element.h: the rule the row-deferred launches replay)
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// ---- RMSProp and SGD: the same grid (chunks of 4096 elements, tensors) and the same clip scale as the Adam kernel ------------
struct SgdArgs {
  float* p[RELGNN_MT_MAX];
  const float* g[RELGNN_MT_MAX];
  long long n[RELGNN_MT_MAX];
};

// g' = g * scale, then TF1 ApplyRMSProp in the operation order of oracle/optim.py:
//   ms += (g'*g' - ms) * (1 - decay);  mom = mom*momentum + lr*g'/sqrt(ms + eps);  p -= mom
// THE element rule: every product and sum is rounded on its own (no contraction, whatever the compile flags say), so an element's
// new bits depend on its own (p, g, ms, mom) and the scalars only — not on its position, the tensor's length, or which loop ran it.
__device__ __forceinline__ void rmsprop_element(float& p, float g, float& ms, float& mom, float scale, float lr,
                                                float one_minus_decay, float momentum, float eps) {
#pragma clang fp contract(off)
  const float gi = g * scale;
  const float d = gi * gi - ms;
  ms = ms + d * one_minus_decay;
  const float num = lr * gi;
  mom = mom * momentum + num / sqrtf(ms + eps);
  p = p - mom;
}

// g' = g * scale, then ApplyGradientDescent: p -= lr*g'
__device__ __forceinline__ void sgd_element(float& p, float g, float scale, float lr) {
#pragma clang fp contract(off)
  const float gi = g * scale;
  p = p - lr * gi;
}

__device__ __forceinline__ float clip_scale(const float* __restrict__ norms, int t, float clip) {
  return clip > 0.f ? clip / fmaxf(norms[t], clip) : 1.f;      // exactly 1 where nothing is clipped (norm 0 included)
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

__global__ __launch_bounds__(256) void mt_rmsprop_clip_kernel(MtArgs a, const float* __restrict__ norms, float clip, float lr,
                                                              float decay, float momentum, float eps) {
  const int t = blockIdx.y;
  const long long n = a.n[t];
  const long long beg = (long long)blockIdx.x * 4096;
  if (beg >= n) return;
  const int len = (int)min(n - beg, 4096LL);
  const float scale = clip_scale(norms, t, clip);
  const float omd = 1.f - decay;
  float* p = a.p[t] + beg;                 // (m, v of MtArgs: the mean-square and the momentum slot)
  const float* g = a.g[t] + beg;
  float* ms = a.m[t] + beg;
  float* mom = a.v[t] + beg;
  // 16-byte loads and stores over the body when all four tensors allow them (beg is a multiple of 4096 elements: the bases decide;
  // a parameter may be a view that starts at a 4-byte offset), scalar code otherwise and for the tail
  const int n4 = aligned16(p, g, ms, mom) ? len / 4 : 0;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], sv = reinterpret_cast<float4*>(ms)[i], mv = reinterpret_cast<float4*>(mom)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    rmsprop_element(pv.x, gv.x, sv.x, mv.x, scale, lr, omd, momentum, eps);
    rmsprop_element(pv.y, gv.y, sv.y, mv.y, scale, lr, omd, momentum, eps);
    rmsprop_element(pv.z, gv.z, sv.z, mv.z, scale, lr, omd, momentum, eps);
    rmsprop_element(pv.w, gv.w, sv.w, mv.w, scale, lr, omd, momentum, eps);
    reinterpret_cast<float4*>(ms)[i] = sv;
    reinterpret_cast<float4*>(mom)[i] = mv;
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  for (int i = 4 * n4 + threadIdx.x; i < len; i += blockDim.x) {
    float pi = p[i], si = ms[i], mi = mom[i];
    rmsprop_element(pi, g[i], si, mi, scale, lr, omd, momentum, eps);
    ms[i] = si;
    mom[i] = mi;
    p[i] = pi;
  }
}

__global__ __launch_bounds__(256) void mt_sgd_clip_kernel(SgdArgs a, const float* __restrict__ norms, float clip, float lr) {
  const int t = blockIdx.y;
  const long long n = a.n[t];
  const long long beg = (long long)blockIdx.x * 4096;
  if (beg >= n) return;
  const int len = (int)min(n - beg, 4096LL);
  const float scale = clip_scale(norms, t, clip);
  float* p = a.p[t] + beg;
  const float* g = a.g[t] + beg;
  const int n4 = aligned16(p, g) ? len / 4 : 0;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    sgd_element(pv.x, gv.x, scale, lr);
    sgd_element(pv.y, gv.y, scale, lr);
    sgd_element(pv.z, gv.z, scale, lr);
    sgd_element(pv.w, gv.w, scale, lr);
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  for (int i = 4 * n4 + threadIdx.x; i < len; i += blockDim.x) {
    float pi = p[i];
    sgd_element(pi, g[i], scale, lr);
    p[i] = pi;
  }
}

// ---- PPI head: sigmoid cross-entropy sum + micro-F1 counts -------------------------------------
// stats = {sum of losses, true_pos, false_pos, false_neg, micro-F1, mean_scale * sum of losses}
struct CeAcc {
  double loss;
  int tp, fp, fn;
};

__device__ __forceinline__ void ce_element(float x, float z, CeAcc& a) {
  // tf.nn.sigmoid_cross_entropy_with_logits: max(x,0) - x*z + log(1 + exp(-|x|))
  const float e = expf(-fabsf(x));
  a.loss += (double)(fmaxf(x, 0.f) - x * z + log1pf(e));
  // round(sigmoid(x)) with round-half-even == (1 / (1 + exp(-x)) > 0.5).  For x <= 0, exp(-x) >= 1 makes the quotient
  // <= 0.5 in every rounding; for x > 0, exp(-x) is the e above — one exponential serves the loss and the prediction.
  const bool pred = sigmoid_label(x, e);      // (common.h: the rule relgnn_predict_sigmoid_f32 writes its labels by)
  const int zi = (int)z;
  a.tp += (pred && zi != 0) ? 1 : 0;
  a.fp += (pred && zi != 1) ? 1 : 0;
  a.fn += (!pred && zi != 0) ? 1 : 0;
}

__global__ __launch_bounds__(1024) void sigmoid_ce_stats_kernel(const float* __restrict__ logits,
                                                                const float* __restrict__ labels, long long n,
                                                                double* __restrict__ partial) {
  __shared__ double red[16];
  CeAcc a = {0.0, 0, 0, 0};
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  // 16-byte loads over the aligned body (both arrays are whole allocations), scalar tail
  const bool vec = ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(labels)) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  const float4* x4 = reinterpret_cast<const float4*>(logits);
  const float4* z4 = reinterpret_cast<const float4*>(labels);
  for (long long i = tid; i < n4; i += nth) {
    const float4 x = x4[i], z = z4[i];
    ce_element(x.x, z.x, a); ce_element(x.y, z.y, a); ce_element(x.z, z.z, a); ce_element(x.w, z.w, a);
  }
  for (long long i = 4 * n4 + tid; i < n; i += nth) ce_element(logits[i], labels[i], a);
  double s;
  s = block_sum_1024(a.loss, red);       if (threadIdx.x == 0) partial[blockIdx.x * 4 + 0] = s;
  s = block_sum_1024((double)a.tp, red); if (threadIdx.x == 0) partial[blockIdx.x * 4 + 1] = s;
  s = block_sum_1024((double)a.fp, red); if (threadIdx.x == 0) partial[blockIdx.x * 4 + 2] = s;
  s = block_sum_1024((double)a.fn, red); if (threadIdx.x == 0) partial[blockIdx.x * 4 + 3] = s;
}

// 256 threads: thread b holds the four partial sums of block b; fixed-shape tree reduction
__global__ __launch_bounds__(256) void sigmoid_ce_stats_final_kernel(const double* __restrict__ partial, int nblk,
                                                                     float mean_scale, float* __restrict__ stats) {
  __shared__ double red[4][4];
  __shared__ double tot[4];
  const int b = threadIdx.x;
  double v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = b < nblk ? partial[b * 4 + k] : 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
  }
  const int wave = b >> 6, lane = b & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (b < 4) {
    const double s = (red[0][b] + red[1][b]) + (red[2][b] + red[3][b]);
    stats[b] = (float)s;
    tot[b] = s;
  }
  __syncthreads();
  if (b == 0) {
    // utils/utils.py:70-74: int64 counts, float64 true division, cast to float32
    const double precision = tot[1] / (tot[1] + tot[2]);
    const double recall = tot[1] / (tot[1] + tot[3]);
    stats[4] = (float)((2.0 * precision * recall) / (precision + recall));
    stats[5] = (float)tot[0] * mean_scale;      // float32 product, as tf.reduce_sum(...) / num_nodes would round it
  }
}

// glogits = gs * (sigmoid(x) - z),  gs = g_mean[0] * mean_scale + g_total[0]  (either pointer may be null)
__global__ __launch_bounds__(256) void sigmoid_ce_bwd_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ labels, long long n,
                                                             const float* __restrict__ g_mean, float mean_scale,
                                                             const float* __restrict__ g_total, float* __restrict__ gl) {
  float gs = 0.f;
  if (g_mean) gs = g_mean[0] * mean_scale;
  if (g_total) gs = g_mean ? gs + g_total[0] : g_total[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float x = logits[i];
    gl[i] = gs * (1.f / (1.f + expf(-x)) - labels[i]);
  }
}

// the same gradient into rows of ldg >= cols floats, the columns behind `cols` written as zeros: the operand of an input-gradient
// product whose reduction length (cols = 121 labels) is then a multiple of 16 (relgnn_limb_gemm_xf32 over ldg columns)
__global__ __launch_bounds__(256) void sigmoid_ce_bwd_padded_kernel(const float* __restrict__ logits,
                                                                    const float* __restrict__ labels, long long rows, int cols,
                                                                    int ldg, const float* __restrict__ g_mean, float mean_scale,
                                                                    const float* __restrict__ g_total, float* __restrict__ gl) {
  float gs = 0.f;
  if (g_mean) gs = g_mean[0] * mean_scale;
  if (g_total) gs = g_mean ? gs + g_total[0] : g_total[0];
  const long long n = rows * ldg;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / ldg;
    const int c = (int)(i - r * ldg);
    float v = 0.f;
    if (c < cols) {
      const float x = logits[r * cols + c];
      v = gs * (1.f / (1.f + expf(-x)) - labels[r * cols + c]);
    }
    gl[i] = v;
  }
}

// ---- citation head: masked sparse softmax cross-entropy + accuracy (tasks/citation_network_task.py:133-148) -----------
// stats = {sum_v loss_v mask_v, sum_v mask_v, sum_v [argmax_v == label_v] mask_v, stats[0] / stats[1], stats[2] / stats[1]}
// One row of logits belongs to a GROUP of W lanes (W = 1, 16 or 64, chosen from cols by the host: the datasets have 3-7 classes,
// a wave then takes 64 rows at once instead of one); lane j of the group walks columns j, j + W, ... with a running
// (maximum, sum of exp(x - maximum) over the other columns, index of the first maximum), and the W partial triples are merged by a butterfly.
// (RowLse, lse_push, lse_merge, row_lse<W> and softmax_group_width live in common.h: predict.hip takes its class from the same code)

// grid-strided over groups of rows; every lane of a wave runs the same number of iterations (the butterfly needs all lanes), a
// lane past the last row walks zero columns.  partial[block * 3 + {0, 1, 2}] = the block's sums in double.
template <int W>
__global__ __launch_bounds__(256) void softmax_ce_stats_kernel(const float* __restrict__ logits, long long ld,
                                                               const int* __restrict__ labels, const float* __restrict__ mask,
                                                               long long rows, int cols, double* __restrict__ partial) {
  __shared__ double red[16];
  constexpr int kRowsPerBlock = 256 / W;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  double loss = 0.0, msum = 0.0, correct = 0.0;
  for (long long base = (long long)blockIdx.x * kRowsPerBlock; base < rows; base += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = base + g;
    const bool valid = r < rows;
    const float* row = logits + (valid ? r : 0) * ld;
    const RowLse a = row_lse<W>(row, valid ? cols : 0, j);
    if (valid && j == 0) {
      const int label = labels[r];
      const float mk = mask[r];
      const float xl = (label >= 0 && label < cols) ? row[label] : a.m;      // (a label outside the row: no access, loss unspecified)
      // log-sum-exp in fp32 as TF's kernel; the (max - x_label) part and everything summed over rows in double
      const double l = (double)log1pf(a.t) + (xl == a.m ? 0.0 : (double)a.m - (double)xl);      // (equal: also -inf next to -inf)
      loss += l * (double)mk;
      msum += (double)mk;
      correct += a.idx == label ? (double)mk : 0.0;
    }
  }
  double s;
  s = block_sum_1024(loss, red);    if (threadIdx.x == 0) partial[blockIdx.x * 3 + 0] = s;
  s = block_sum_1024(msum, red);    if (threadIdx.x == 0) partial[blockIdx.x * 3 + 1] = s;
  s = block_sum_1024(correct, red); if (threadIdx.x == 0) partial[blockIdx.x * 3 + 2] = s;
}

// 256 threads: thread b holds the partial sums of block b (nblk may be 0: no rows); fixed-shape tree reduction.  The loss is divided
// by the sum of the mask, or (weighted) by the caller's denominator.
template <bool kWeighted>
__device__ __forceinline__ void softmax_ce_stats_tree(const double* __restrict__ partial, int nblk, float denominator,
                                                      float* __restrict__ stats) {
  constexpr int kSums = kWeighted ? 4 : 3;
  __shared__ double red[4][kSums];
  const int b = threadIdx.x;
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = b < nblk ? partial[b * kSums + k] : 0.0;
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
  }
  const int wave = b >> 6, lane = b & 63;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (b == 0) {
    float t[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) t[k] = (float)((red[0][k] + red[1][k]) + (red[2][k] + red[3][k]));
#pragma unroll
    for (int k = 0; k < 3; ++k) stats[k] = t[k];
    // float32 quotients of the float32 sums, as the reference's graph forms them (:141, :145); 0 / 0 stays NaN
    if constexpr (kWeighted) stats[3] = t[0] / denominator;
    else stats[3] = t[0] / t[1];
    stats[4] = t[2] / t[1];
    if constexpr (kWeighted) stats[5] = t[3];
  }
}

__global__ __launch_bounds__(256) void softmax_ce_stats_final_kernel(const double* __restrict__ partial, int nblk,
                                                                     float* __restrict__ stats) {
  softmax_ce_stats_tree<false>(partial, nblk, 0.f, stats);
}

// glogits[v, c] = mask_v * (softmax(logits_v)_c - [c == label_v]) * (g_total[0] + g_loss[0] / stats[1]) for c < cols, 0 for
// cols <= c < ldg; a row with mask 0 is written as zeros whatever its logits hold.  Either gradient pointer may be null.
template <int W>
__global__ __launch_bounds__(256) void softmax_ce_bwd_kernel(const float* __restrict__ logits, long long ld,
                                                             const int* __restrict__ labels, const float* __restrict__ mask,
                                                             long long rows, int cols, const float* __restrict__ stats,
                                                             const float* __restrict__ g_loss, const float* __restrict__ g_total,
                                                             float* __restrict__ gl, long long ldg) {
  constexpr int kRowsPerBlock = 256 / W;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  float gs = 0.f;
  if (g_loss) gs = g_loss[0] / stats[1];
  if (g_total) gs = g_loss ? gs + g_total[0] : g_total[0];
  for (long long base = (long long)blockIdx.x * kRowsPerBlock; base < rows; base += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = base + g;
    const bool valid = r < rows;
    const float* row = logits + (valid ? r : 0) * ld;
    const RowLse a = row_lse<W>(row, valid ? cols : 0, j);
    if (!valid) continue;
    const float mk = mask[r];
    const int label = labels[r];
    const float scale = mk * gs, inv = 1.f / (1.f + a.t);
    float* out = gl + r * ldg;
    for (int c = j; c < (int)ldg; c += W) {
      float v = 0.f;
      if (c < cols && mk != 0.f) v = scale * (expf(row[c] - a.m) * inv - (c == label ? 1.f : 0.f));
      out[c] = v;
    }
  }
}

// ---- the same head with a weight per row (include/relgnn_subgraph_norm.h: GraphSAINT's loss normalisation) ------------------------
// stats = {sum_v loss_v mask_v weight_v, sum_v mask_v, sum_v [argmax_v == label_v] mask_v, stats[0] / denominator, stats[2] / stats[1],
// sum_v mask_v weight_v}: the row walk, the per-row loss and the order of every sum are softmax_ce_stats_kernel's, so that with every
// weight 1 the first three sums are its bits (mask * 1 and l * (mask * 1) are exact).  partial[block * 4 + {0, 1, 2, 3}].
// (This kernel and softmax_ce_weighted_bwd_kernel keep bodies of their own next to the plain ones: as one inlined function per pair
// hipcc lays the row loop's blocks out differently (profiles/citation_batches.txt).  The final trees and the host wrappers are shared.)
template <int W>
__global__ __launch_bounds__(256) void softmax_ce_weighted_stats_kernel(const float* __restrict__ logits, long long ld,
                                                                        const int* __restrict__ labels, const float* __restrict__ mask,
                                                                        const float* __restrict__ weights, long long rows, int cols,
                                                                        double* __restrict__ partial) {
  __shared__ double red[16];
  constexpr int kRowsPerBlock = 256 / W;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  double loss = 0.0, msum = 0.0, correct = 0.0, wsum = 0.0;
  for (long long base = (long long)blockIdx.x * kRowsPerBlock; base < rows; base += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = base + g;
    const bool valid = r < rows;
    const float* row = logits + (valid ? r : 0) * ld;
    const RowLse a = row_lse<W>(row, valid ? cols : 0, j);
    if (valid && j == 0) {
      const int label = labels[r];
      const float mk = mask[r];
      const double mw = (double)mk * (double)weights[r];
      const float xl = (label >= 0 && label < cols) ? row[label] : a.m;
      const double l = (double)log1pf(a.t) + (xl == a.m ? 0.0 : (double)a.m - (double)xl);
      loss += l * mw;
      msum += (double)mk;
      correct += a.idx == label ? (double)mk : 0.0;
      wsum += mw;
    }
  }
  double s;
  s = block_sum_1024(loss, red);    if (threadIdx.x == 0) partial[blockIdx.x * 4 + 0] = s;
  s = block_sum_1024(msum, red);    if (threadIdx.x == 0) partial[blockIdx.x * 4 + 1] = s;
  s = block_sum_1024(correct, red); if (threadIdx.x == 0) partial[blockIdx.x * 4 + 2] = s;
  s = block_sum_1024(wsum, red);    if (threadIdx.x == 0) partial[blockIdx.x * 4 + 3] = s;
}

// softmax_ce_stats_tree over four sums; the loss is divided by the caller's denominator, not by the sum of the mask
__global__ __launch_bounds__(256) void softmax_ce_weighted_stats_final_kernel(const double* __restrict__ partial, int nblk,
                                                                              float denominator, float* __restrict__ stats) {
  softmax_ce_stats_tree<true>(partial, nblk, denominator, stats);
}

// glogits[v, c] = mask_v * weight_v * (softmax(logits_v)_c - [c == label_v]) * (g_total[0] + g_loss[0] / denominator) for c < cols, 0
// for cols <= c < ldg; a row with mask 0 is written as zeros.  Either gradient pointer may be null.
template <int W>
__global__ __launch_bounds__(256) void softmax_ce_weighted_bwd_kernel(const float* __restrict__ logits, long long ld,
                                                                      const int* __restrict__ labels, const float* __restrict__ mask,
                                                                      const float* __restrict__ weights, float denominator,
                                                                      long long rows, int cols, const float* __restrict__ g_loss,
                                                                      const float* __restrict__ g_total, float* __restrict__ gl,
                                                                      long long ldg) {
  constexpr int kRowsPerBlock = 256 / W;
  const int j = threadIdx.x % W, g = threadIdx.x / W;
  float gs = 0.f;
  if (g_loss) gs = g_loss[0] / denominator;
  if (g_total) gs = g_loss ? gs + g_total[0] : g_total[0];
  for (long long base = (long long)blockIdx.x * kRowsPerBlock; base < rows; base += (long long)gridDim.x * kRowsPerBlock) {
    const long long r = base + g;
    const bool valid = r < rows;
    const float* row = logits + (valid ? r : 0) * ld;
    const RowLse a = row_lse<W>(row, valid ? cols : 0, j);
    if (!valid) continue;
    const float mk = mask[r];
    const int label = labels[r];
    const float scale = (mk * weights[r]) * gs, inv = 1.f / (1.f + a.t);
    float* out = gl + r * ldg;
    for (int c = j; c < (int)ldg; c += W) {
      float v = 0.f;
      if (c < cols && mk != 0.f) v = scale * (expf(row[c] - a.m) * inv - (c == label ? 1.f : 0.f));
      out[c] = v;
    }
  }
}

constexpr int kSoftmaxBlocks = 256;

static inline int softmax_grid(long long rows, int w) {
  const long long per_block = 256 / w;
  long long g = (rows + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > kSoftmaxBlocks ? kSoftmaxBlocks : g));
}

// The argument checks, the grid and the W dispatch of both heads' entry points (kWeighted: the weights must be there, the denominator
// a number other than 0, and the workspace holds four sums a block).
template <bool kWeighted>
int softmax_ce_stats_launch(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                            float denominator, int64_t rows, int32_t cols, float* stats, void* workspace, size_t workspace_bytes,
                            void* stream) {
  if (rows < 0 || cols < 1 || ld < cols || !stats || (kWeighted && (denominator == 0.f || denominator != denominator)))
    return RELGNN_EINVAL;
  if (!workspace || workspace_bytes < (size_t)kSoftmaxBlocks * (kWeighted ? 4 : 3) * sizeof(double)) return RELGNN_ENOSPC;
  if (rows > 0 && (!logits || !labels || !mask || (kWeighted && !weights))) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  int nblk = 0;
  if (rows > 0) {
    const int w = softmax_group_width(cols);
    nblk = softmax_grid(rows, w);
    auto walk = [&](auto width) {
      constexpr int W = decltype(width)::value;
      if constexpr (kWeighted) softmax_ce_weighted_stats_kernel<W><<<nblk, 256, 0, st>>>(logits, ld, labels, mask, weights, rows, cols, partial);
      else softmax_ce_stats_kernel<W><<<nblk, 256, 0, st>>>(logits, ld, labels, mask, rows, cols, partial);
    };
    if (w == 1) walk(std::integral_constant<int, 1>{});
    else if (w == 16) walk(std::integral_constant<int, 16>{});
    else walk(std::integral_constant<int, 64>{});
  }
  if constexpr (kWeighted) softmax_ce_weighted_stats_final_kernel<<<1, 256, 0, st>>>(partial, nblk, denominator, stats);
  else softmax_ce_stats_final_kernel<<<1, 256, 0, st>>>(partial, nblk, stats);
  return launch_status();
}

template <bool kWeighted>
int softmax_ce_bwd_launch(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                          float denominator, int64_t rows, int32_t cols, const float* stats, const float* g_loss,
                          const float* g_total, float* glogits, int64_t ldg, void* stream) {
  if (rows < 0 || cols < 1 || ld < cols || ldg < cols || ldg > INT32_MAX
      || (kWeighted && (denominator == 0.f || denominator != denominator)))
    return RELGNN_EINVAL;
  if (rows == 0) return RELGNN_OK;
  if (!logits || !labels || !mask || (kWeighted ? !weights : !stats) || (!g_loss && !g_total) || !glogits) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  const int w = softmax_group_width(cols);
  const int64_t per_block = 256 / w;
  const unsigned nblk = flat_grid((rows + per_block - 1) / per_block * 256, 256);       // one block per 256 / w rows, capped
  auto walk = [&](auto width) {
    constexpr int W = decltype(width)::value;
    if constexpr (kWeighted)
      softmax_ce_weighted_bwd_kernel<W><<<nblk, 256, 0, st>>>(logits, ld, labels, mask, weights, denominator, rows, cols, g_loss, g_total, glogits, ldg);
    else
      softmax_ce_bwd_kernel<W><<<nblk, 256, 0, st>>>(logits, ld, labels, mask, rows, cols, stats, g_loss, g_total, glogits, ldg);
  };
  if (w == 1) walk(std::integral_constant<int, 1>{});
  else if (w == 16) walk(std::integral_constant<int, 16>{});
  else walk(std::integral_constant<int, 64>{});
  return launch_status();
}

constexpr int kStatsBlocks = 256;

}  // namespace

extern "C" {

size_t relgnn_mt_l2norm_workspace_bytes(void) { return (size_t)RELGNN_MT_MAX * kNormChunks * sizeof(double); }

int relgnn_mt_l2norm(const float* const* h_grads, const int64_t* h_sizes, int32_t n, float* norms, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (n < 0 || n > RELGNN_MT_MAX) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!h_grads || !h_sizes || !norms) return RELGNN_EINVAL;
  if (!workspace || workspace_bytes < relgnn_mt_l2norm_workspace_bytes()) return RELGNN_ENOSPC;
  NormArgs a;
  for (int i = 0; i < n; ++i) {
    if (h_sizes[i] < 0 || (h_sizes[i] > 0 && !h_grads[i])) return RELGNN_EINVAL;
    a.g[i] = h_grads[i];
    a.n[i] = h_sizes[i];
  }
  double* partial = static_cast<double*>(workspace);
  mt_l2norm_partial_kernel<<<dim3(kNormChunks, (unsigned)n), kNormBlock, 0, as_stream(stream)>>>(a, partial);
  mt_l2norm_final_kernel<<<n, 64, 0, as_stream(stream)>>>(partial, norms);
  return launch_status();
}

int relgnn_adam_step_size(float* d_state, float lr, float beta1, float beta2, void* stream) {
  if (!d_state) return RELGNN_EINVAL;
  adam_step_size_kernel<<<1, 1, 0, as_stream(stream)>>>(d_state, lr, beta1, beta2);
  return launch_status();
}

static int mt_adam_clip_impl(float* const* h_params, const float* const* h_grads, float* const* h_m, float* const* h_v,
                             const int64_t* h_sizes, int32_t n, const float* norms, float clip, float lr_t,
                             const float* d_lr_t, float beta1, float beta2, float eps, void* stream);

int relgnn_mt_adam_clip(float* const* h_params, const float* const* h_grads, float* const* h_m, float* const* h_v,
                        const int64_t* h_sizes, int32_t n, const float* norms, float clip, float lr_t, float beta1,
                        float beta2, float eps, void* stream) {
  return mt_adam_clip_impl(h_params, h_grads, h_m, h_v, h_sizes, n, norms, clip, lr_t, nullptr, beta1, beta2, eps, stream);
}

int relgnn_mt_adam_clip_devlr(float* const* h_params, const float* const* h_grads, float* const* h_m, float* const* h_v,
                              const int64_t* h_sizes, int32_t n, const float* norms, float clip, const float* d_lr_t,
                              float beta1, float beta2, float eps, void* stream) {
  if (!d_lr_t) return RELGNN_EINVAL;
  return mt_adam_clip_impl(h_params, h_grads, h_m, h_v, h_sizes, n, norms, clip, 0.f, d_lr_t, beta1, beta2, eps, stream);
}

static int mt_adam_clip_impl(float* const* h_params, const float* const* h_grads, float* const* h_m, float* const* h_v,
                             const int64_t* h_sizes, int32_t n, const float* norms, float clip, float lr_t,
                             const float* d_lr_t, float beta1, float beta2, float eps, void* stream) {
  if (n < 0 || n > RELGNN_MT_MAX) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!h_params || !h_grads || !h_m || !h_v || !h_sizes || (clip > 0.f && !norms)) return RELGNN_EINVAL;
  MtArgs a;
  long long maxn = 0;
  for (int i = 0; i < n; ++i) {
    if (h_sizes[i] < 0) return RELGNN_EINVAL;
    a.p[i] = h_params[i]; a.g[i] = h_grads[i]; a.m[i] = h_m[i]; a.v[i] = h_v[i]; a.n[i] = h_sizes[i];
    if (h_sizes[i] > maxn) maxn = h_sizes[i];
  }
  if (maxn == 0) return RELGNN_OK;
  dim3 grid((unsigned)((maxn + 4095) / 4096), (unsigned)n);
  mt_adam_clip_kernel<<<grid, 256, 0, as_stream(stream)>>>(a, norms, clip, lr_t, d_lr_t, beta1, beta2, eps);
  return launch_status();
}

int relgnn_mt_rmsprop_clip(float* const* h_params, const float* const* h_grads, float* const* h_ms, float* const* h_mom,
                           const int64_t* h_sizes, int32_t n, const float* norms, float clip, float lr, float decay,
                           float momentum, float eps, void* stream) {
  if (n < 0 || n > RELGNN_MT_MAX) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!h_params || !h_grads || !h_ms || !h_mom || !h_sizes || (clip > 0.f && !norms)) return RELGNN_EINVAL;
  MtArgs a;
  long long maxn = 0;
  for (int i = 0; i < n; ++i) {
    if (h_sizes[i] < 0 || (h_sizes[i] > 0 && (!h_params[i] || !h_grads[i] || !h_ms[i] || !h_mom[i]))) return RELGNN_EINVAL;
    a.p[i] = h_params[i]; a.g[i] = h_grads[i]; a.m[i] = h_ms[i]; a.v[i] = h_mom[i]; a.n[i] = h_sizes[i];
    if (h_sizes[i] > maxn) maxn = h_sizes[i];
  }
  if (maxn == 0) return RELGNN_OK;
  dim3 grid((unsigned)((maxn + 4095) / 4096), (unsigned)n);
  mt_rmsprop_clip_kernel<<<grid, 256, 0, as_stream(stream)>>>(a, norms, clip, lr, decay, momentum, eps);
  return launch_status();
}

int relgnn_mt_sgd_clip(float* const* h_params, const float* const* h_grads, const int64_t* h_sizes, int32_t n,
                       const float* norms, float clip, float lr, void* stream) {
  if (n < 0 || n > RELGNN_MT_MAX) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!h_params || !h_grads || !h_sizes || (clip > 0.f && !norms)) return RELGNN_EINVAL;
  SgdArgs a;
  long long maxn = 0;
  for (int i = 0; i < n; ++i) {
    if (h_sizes[i] < 0 || (h_sizes[i] > 0 && (!h_params[i] || !h_grads[i]))) return RELGNN_EINVAL;
    a.p[i] = h_params[i]; a.g[i] = h_grads[i]; a.n[i] = h_sizes[i];
    if (h_sizes[i] > maxn) maxn = h_sizes[i];
  }
  if (maxn == 0) return RELGNN_OK;
  dim3 grid((unsigned)((maxn + 4095) / 4096), (unsigned)n);
  mt_sgd_clip_kernel<<<grid, 256, 0, as_stream(stream)>>>(a, norms, clip, lr);
  return launch_status();
}

size_t relgnn_sigmoid_ce_stats_workspace_bytes(void) { return (size_t)kStatsBlocks * 4 * sizeof(double); }

int relgnn_sigmoid_ce_stats(const float* logits, const float* labels, int64_t n, float mean_scale, float* stats,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (n < 0 || !stats) return RELGNN_EINVAL;
  if (!workspace || workspace_bytes < relgnn_sigmoid_ce_stats_workspace_bytes()) return RELGNN_ENOSPC;
  if (n > 0 && (!logits || !labels)) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  int nblk = (int)((n + 1023) / 1024);
  if (nblk < 1) nblk = 1;
  if (nblk > kStatsBlocks) nblk = kStatsBlocks;
  sigmoid_ce_stats_kernel<<<nblk, 1024, 0, st>>>(logits, labels, n, static_cast<double*>(workspace));
  sigmoid_ce_stats_final_kernel<<<1, 256, 0, st>>>(static_cast<const double*>(workspace), nblk, mean_scale, stats);
  return launch_status();
}

int relgnn_sigmoid_ce_bwd(const float* logits, const float* labels, int64_t n, const float* g_mean, float mean_scale,
                          const float* g_total, float* glogits, void* stream) {
  if (n < 0) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!logits || !labels || (!g_mean && !g_total) || !glogits) return RELGNN_EINVAL;
  sigmoid_ce_bwd_kernel<<<flat_grid(n, 256), 256, 0, as_stream(stream)>>>(logits, labels, n, g_mean, mean_scale, g_total,
                                                                          glogits);
  return launch_status();
}

int relgnn_sigmoid_ce_bwd_padded(const float* logits, const float* labels, int64_t rows, int32_t cols, const float* g_mean,
                                 float mean_scale, const float* g_total, float* glogits, int32_t ldg, void* stream) {
  if (rows < 0 || cols < 0 || ldg < cols) return RELGNN_EINVAL;
  if (rows == 0 || ldg == 0) return RELGNN_OK;
  if (!logits || !labels || (!g_mean && !g_total) || !glogits) return RELGNN_EINVAL;
  sigmoid_ce_bwd_padded_kernel<<<flat_grid(rows * ldg, 256), 256, 0, as_stream(stream)>>>(logits, labels, rows, cols, ldg, g_mean,
                                                                                          mean_scale, g_total, glogits);
  return launch_status();
}

size_t relgnn_softmax_ce_stats_workspace_bytes(void) { return (size_t)kSoftmaxBlocks * 3 * sizeof(double); }

int relgnn_softmax_ce_stats(const float* logits, int64_t ld, const int32_t* labels, const float* mask, int64_t rows, int32_t cols,
                            float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  return softmax_ce_stats_launch<false>(logits, ld, labels, mask, nullptr, 0.f, rows, cols, stats, workspace, workspace_bytes, stream);
}

int relgnn_softmax_ce_bwd(const float* logits, int64_t ld, const int32_t* labels, const float* mask, int64_t rows, int32_t cols,
                          const float* stats, const float* g_loss, const float* g_total, float* glogits, int64_t ldg,
                          void* stream) {
  return softmax_ce_bwd_launch<false>(logits, ld, labels, mask, nullptr, 0.f, rows, cols, stats, g_loss, g_total, glogits, ldg, stream);
}

size_t relgnn_softmax_ce_weighted_stats_workspace_bytes(void) { return (size_t)kSoftmaxBlocks * 4 * sizeof(double); }

int relgnn_softmax_ce_weighted_stats(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                                     float denominator, int64_t rows, int32_t cols, float* stats, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return softmax_ce_stats_launch<true>(logits, ld, labels, mask, weights, denominator, rows, cols, stats, workspace, workspace_bytes,
                                       stream);
}

int relgnn_softmax_ce_weighted_bwd(const float* logits, int64_t ld, const int32_t* labels, const float* mask, const float* weights,
                                   float denominator, int64_t rows, int32_t cols, const float* g_loss, const float* g_total,
                                   float* glogits, int64_t ldg, void* stream) {
  return softmax_ce_bwd_launch<true>(logits, ld, labels, mask, weights, denominator, rows, cols, nullptr, g_loss, g_total, glogits, ldg,
                                     stream);
}

}  // extern "C"
