// VarMisuse task (tasks/varmisuse_task.py of the reference): the task-owned input model and the per-graph output head.
//   * character CNN over node labels                  tasks/varmisuse_task.py:317-367
//       one_hot(68) -> Conv1D(16, 5, leaky_relu) -> MaxPool1D(5, 1) -> Conv1D(D, C - 8, leaky_relu) -> squeeze -> gather
//   * slot / candidate head, loss, accuracy           tasks/varmisuse_task.py:369-448
// Deterministic: no float atomics; every sum has a fixed order.  A label's forward arithmetic is the same chain of operations
// whatever its row number and the number of labels, so the same label gives the same bits everywhere.
#include "common.h"

using namespace relgnn;

namespace {

constexpr int kAlphabet = 68;                        // len(ALPHABET), :15: codes 0 .. 67 are live one-hot columns, 68 and up all-zero rows
constexpr int kK1 = 5, kF1 = 16;                     // first convolution: kernel 5, 16 filters (hard-wired at :346-354)
constexpr int kW1Floats = kK1 * kAlphabet * kF1;     // 5440
constexpr int kMinC = 9, kMaxC = 32, kMaxD = 128;
constexpr int kMaxT1 = kMaxC - 4, kMaxK2 = kMaxC - 8;
constexpr int kFwdTile = 8;                          // labels per workgroup iteration of the forward
constexpr int kBwdTile = 4;                          // labels per workgroup iteration of the backward
constexpr int kBwdRange = 64;                        // smallest label range one workgroup of the backward owns
constexpr int kBwdMaxBlocks = 512;
constexpr int kPartialStride = kW1Floats + kF1;      // one workgroup's partial table: dW1 then db1

__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : 0.2f * x; }

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: persistent workgroups; W1 (21.8 KB) staged once in LDS, labels streamed through in tiles of kFwdTile
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void charcnn_fwd_kernel(const uint8_t* __restrict__ chars, long long U, int C, int D,
                                                          const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ W2, const float* __restrict__ b2,
                                                          float* __restrict__ out) {
  __shared__ float sW1[kW1Floats];
  __shared__ float sB1[kF1];
  __shared__ uint8_t sC[kFwdTile][kMaxC];
  __shared__ float sZ[kFwdTile][kMaxT1][kF1];
  __shared__ float sP[kFwdTile][kMaxK2 * kF1];
  const int tid = threadIdx.x;
  const int T1 = C - 4, K2 = C - 8, KF = K2 * kF1;
  for (int i = tid; i < kW1Floats; i += 256) sW1[i] = W1[i];
  if (tid < kF1) sB1[tid] = b1[tid];
  const long long ntiles = (U + kFwdTile - 1) / kFwdTile;
  const int groups = 256 / D;                        // D <= 128: at least two groups of D threads
  const int grp = tid / D, d = tid % D;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();                                 // W1 is staged / the previous tile's buffers are free
    const long long base = tile * kFwdTile;
    const int nl = (int)((U - base) < kFwdTile ? (U - base) : kFwdTile);
    for (int i = tid; i < nl * C; i += 256) sC[i / C][i % C] = chars[base * C + i];
    __syncthreads();
    // conv1[l, t, f] = b1[f] + sum_j W1[j, c[l, t + j], f]: the one-hot product as a table lookup
    for (int i = tid; i < nl * T1 * kF1; i += 256) {
      const int f = i & (kF1 - 1), t = (i >> 4) % T1, l = (i >> 4) / T1;
      float acc = sB1[f];
#pragma unroll
      for (int j = 0; j < kK1; ++j) {
        const int code = sC[l][t + j];
        if (code < kAlphabet) acc += sW1[(j * kAlphabet + code) * kF1 + f];
      }
      sZ[l][t][f] = leaky(acc);
    }
    __syncthreads();
    for (int i = tid; i < nl * K2 * kF1; i += 256) {
      const int f = i & (kF1 - 1), k = (i >> 4) % K2, l = (i >> 4) / K2;
      float m = sZ[l][k][f];
#pragma unroll
      for (int j = 1; j < kK1; ++j) m = fmaxf(m, sZ[l][k + j][f]);
      sP[l][k * kF1 + f] = m;
    }
    __syncthreads();
    // conv2[l, d] = b2[d] + sum_{k, f} pooled[l, k, f] * W2[k, f, d]; group g of D threads owns labels g, g + groups, ...
    if (grp < groups) {
      float acc[4];
      const float bias = b2[d];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = bias;
      for (int kf = 0; kf < KF; ++kf) {
        const float w = W2[(long long)kf * D + d];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int l = grp + q * groups;
          if (l < nl) acc[q] = fmaf(sP[l][kf], w, acc[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = grp + q * groups;
        if (l < nl) out[(base + l) * D + d] = leaky(acc[q]);
      }
    }
  }
}

// out[v, :] = rep[map[v], :]  (tf.gather, :365-366); a map entry outside [0, U) writes zeros and raises the error flag
__global__ __launch_bounds__(256) void charcnn_gather_kernel(const float* __restrict__ rep, const int* __restrict__ map, long long V,
                                                             long long U, int D, float* __restrict__ out, uint32_t* __restrict__ err) {
  const long long n = V * D;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long v = i / D;
    const int d = (int)(i - v * D);
    const int u = map[v];
    float x = 0.f;
    if (u >= 0 && u < U) x = rep[(long long)u * D + d];
    else if (err != nullptr && d == 0) atomicOr(err, RELGNN_ERRFLAG_INDEX_OUT_OF_RANGE);
    out[i] = x;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: workgroup b owns the labels [b * labels_per_block, (b + 1) * labels_per_block); it recomputes their forward, writes
// the pooled table P [U, K2 * 16] and the second layer's pre-activation gradient G2 [U, D] (operands of dW2 = P^T G2 and
// db2 = column sums of G2), and keeps ITS dW1 / db1 partial table: thread (j, f) is the only writer of the entries (j, *, f), so the
// (j, PAD) rows that receive most contributions cost no more than any other row, and the order of additions is fixed.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void charcnn_bwd_kernel(const uint8_t* __restrict__ chars, long long U, int C, int D,
                                                          const float* __restrict__ W1, const float* __restrict__ b1,
                                                          const float* __restrict__ W2, const float* __restrict__ b2,
                                                          const float* __restrict__ gU, float* __restrict__ P, float* __restrict__ G2,
                                                          double* __restrict__ partial, long long labels_per_block) {
  __shared__ float sT[kW1Floats];
  __shared__ uint8_t sC[kBwdTile][kMaxC];
  __shared__ float sZ[kBwdTile][kMaxT1][kF1];        // first layer's pre-activation, then its gradient
  __shared__ float sP[kBwdTile][kMaxK2 * kF1];
  __shared__ uint8_t sA[kBwdTile][kMaxK2 * kF1];     // offset of the FIRST maximum inside each pooling window
  __shared__ float sG[kBwdTile][kMaxD];
  __shared__ float sDP[kBwdTile][kMaxK2 * kF1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T1 = C - 4, K2 = C - 8, KF = K2 * kF1;
  for (int i = tid; i < kW1Floats; i += 256) sT[i] = 0.f;
  double db1 = 0.0;
  const long long first = (long long)blockIdx.x * labels_per_block;
  const long long last = first + labels_per_block < U ? first + labels_per_block : U;
  for (long long base = first; base < last; base += kBwdTile) {
    __syncthreads();
    const int nl = (int)((last - base) < kBwdTile ? (last - base) : kBwdTile);
    for (int i = tid; i < nl * C; i += 256) sC[i / C][i % C] = chars[base * C + i];
    __syncthreads();
    for (int i = tid; i < nl * T1 * kF1; i += 256) {
      const int f = i & (kF1 - 1), t = (i >> 4) % T1, l = (i >> 4) / T1;
      float acc = b1[f];
#pragma unroll
      for (int j = 0; j < kK1; ++j) {
        const int code = sC[l][t + j];
        if (code < kAlphabet) acc += W1[(j * kAlphabet + code) * kF1 + f];
      }
      sZ[l][t][f] = acc;
    }
    __syncthreads();
    for (int i = tid; i < nl * K2 * kF1; i += 256) {
      const int f = i & (kF1 - 1), k = (i >> 4) % K2, l = (i >> 4) / K2;
      float m = leaky(sZ[l][k][f]);
      int a = 0;
#pragma unroll
      for (int j = 1; j < kK1; ++j) {
        const float v = leaky(sZ[l][k + j][f]);
        if (v > m) { m = v; a = j; }
      }
      sP[l][k * kF1 + f] = m;
      sA[l][k * kF1 + f] = (uint8_t)a;
      P[(base + l) * KF + k * kF1 + f] = m;
    }
    __syncthreads();
    for (int i = tid; i < nl * D; i += 256) {
      const int l = i / D, d = i % D;
      float acc = b2[d];                             // the forward's own chain: the sign of the pre-activation is the forward's
      for (int kf = 0; kf < KF; ++kf) acc = fmaf(sP[l][kf], W2[(long long)kf * D + d], acc);
      const float g = gU[(base + l) * D + d] * (acc > 0.f ? 1.f : 0.2f);
      sG[l][d] = g;
      G2[(base + l) * D + d] = g;
    }
    __syncthreads();
    // d pooled[l, k, f] = sum_d G2[l, d] * W2[k, f, d]: one wave per entry, lanes over d, butterfly sum
    for (int it = wave; it < nl * KF; it += 4) {
      const int l = it / KF, kf = it % KF;
      float s = 0.f;
      for (int d = lane; d < D; d += 64) s = fmaf(sG[l][d], W2[(long long)kf * D + d], s);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) sDP[l][kf] = s;
    }
    __syncthreads();
    // through the max-pool (to the first maximum of every window) and the first leaky_relu
    for (int i = tid; i < nl * T1 * kF1; i += 256) {
      const int f = i & (kF1 - 1), t = (i >> 4) % T1, l = (i >> 4) / T1;
      const float z = sZ[l][t][f];
      float s = 0.f;
      const int k0 = t - (kK1 - 1) > 0 ? t - (kK1 - 1) : 0, k1 = t < K2 - 1 ? t : K2 - 1;
      for (int k = k0; k <= k1; ++k)
        if (sA[l][k * kF1 + f] == t - k) s += sDP[l][k * kF1 + f];
      sZ[l][t][f] = s * (z > 0.f ? 1.f : 0.2f);
    }
    __syncthreads();
    if (tid < kK1 * kF1) {
      const int j = tid / kF1, f = tid % kF1;
      for (int l = 0; l < nl; ++l)
        for (int t = 0; t < T1; ++t) {
          const int code = sC[l][t + j];
          if (code < kAlphabet) sT[(j * kAlphabet + code) * kF1 + f] += sZ[l][t][f];
        }
    } else if (tid >= 128 && tid < 128 + kF1) {
      const int f = tid - 128;
      for (int l = 0; l < nl; ++l)
        for (int t = 0; t < T1; ++t) db1 += (double)sZ[l][t][f];
    }
  }
  __syncthreads();
  double* mine = partial + (long long)blockIdx.x * kPartialStride;
  for (int i = tid; i < kW1Floats; i += 256) mine[i] = (double)sT[i];
  if (tid >= 128 && tid < 128 + kF1) mine[kW1Floats + tid - 128] = db1;
}

// dW1 / db1 = the workgroups' partial tables added in workgroup order, in double
__global__ __launch_bounds__(256) void charcnn_bwd_combine_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ dW1,
                                                                  float* __restrict__ db1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kPartialStride) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(long long)b * kPartialStride + i];
  if (i < kW1Floats) dW1[i] = (float)s;
  else db1[i - kW1Floats] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// head: one wave per graph
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxCn = kMaxCandidates, kHeadMaxD = 256, kHeadBlocks = 64;      // (8: common.h, candidate_choice)

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

struct HeadRows {
  long long slot;
  long long cand[kMaxCn];
  bool ok;
};

__device__ __forceinline__ HeadRows head_rows(const int* __restrict__ slot_ids, const int* __restrict__ cand_ids,
                                              const int* __restrict__ first_node, long long g, int Cn, long long V) {
  HeadRows r;
  const long long off = first_node ? (long long)first_node[g] : 0;
  r.slot = off + slot_ids[g];
  r.ok = r.slot >= 0 && r.slot < V;
#pragma unroll
  for (int c = 0; c < kMaxCn; ++c) {
    r.cand[c] = c < Cn ? off + cand_ids[g * Cn + c] : 0;
    r.ok = r.ok && r.cand[c] >= 0 && r.cand[c] < V;
  }
  return r;
}

// logits[g, c] for the wave's graph, in every lane (the pieces the backward needs as well: ip)
template <int NV>
__device__ __forceinline__ void head_logits(const float* __restrict__ H, long long ld, const HeadRows& r, int Cn, int D,
                                            const float* __restrict__ w, const float* __restrict__ mask, long long g, int lane,
                                            float (&s)[NV], float (&cv)[kMaxCn][NV], float (&ip)[kMaxCn], float (&logit)[kMaxCn]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) s[q] = lane + 64 * q < D ? H[r.slot * ld + lane + 64 * q] : 0.f;
  float ls = 0.f;
  if (w) {
#pragma unroll
    for (int q = 0; q < NV; ++q)
      if (lane + 64 * q < D) ls = fmaf(s[q], w[D + lane + 64 * q], ls);
    ls = wave_sum(ls);
  }
#pragma unroll
  for (int c = 0; c < kMaxCn; ++c) {
    ip[c] = 0.f;
    logit[c] = 0.f;
    if (c < Cn) {
      float a = 0.f, lc = 0.f;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const bool in = lane + 64 * q < D;
        cv[c][q] = in ? H[r.cand[c] * ld + lane + 64 * q] : 0.f;
        a = fmaf(s[q], cv[c][q], a);
        if (w && in) lc = fmaf(cv[c][q], w[lane + 64 * q], lc);
      }
      ip[c] = wave_sum(a);
      float x = ip[c];
      if (w) x = (wave_sum(lc) + ls) + ip[c] * w[2 * D];        // [cand | slot | ip] . w  (:404-416)
      logit[c] = x + (1.0f - mask[g * Cn + c]) * -1e7f;           // :420, an addition in float32
    } else {
#pragma unroll
      for (int q = 0; q < NV; ++q) cv[c][q] = 0.f;
    }
  }
}

template <int NV>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ H, long long ld, long long V, int D,
                                                       const int* __restrict__ slot_ids, const int* __restrict__ cand_ids,
                                                       const float* __restrict__ mask, const int* __restrict__ first_node,
                                                       long long G, int Cn, const float* __restrict__ w, float* __restrict__ logits,
                                                       double* __restrict__ per_graph, uint32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const HeadRows r = head_rows(slot_ids, cand_ids, first_node, g, Cn, V);
  if (!r.ok) {                                       // wave-uniform: no row is read, the graph counts for nothing
    if (lane == 0) {
      if (err != nullptr) atomicOr(err, RELGNN_ERRFLAG_INDEX_OUT_OF_RANGE);
      for (int c = 0; c < Cn; ++c) logits[g * Cn + c] = 0.f;
      per_graph[2 * g] = 0.0;
      per_graph[2 * g + 1] = 0.0;
    }
    return;
  }
  float s[NV], cv[kMaxCn][NV], ip[kMaxCn], x[kMaxCn];
  head_logits<NV>(H, ld, r, Cn, D, w, mask, g, lane, s, cv, ip, x);
  if (lane == 0) {
    // maximum, exponentials and tf.argmax(tf.nn.softmax(logits)), the first of equal PROBABILITIES (:438): common.h, the one
    // definition relgnn_predict_candidates_f32 predicts by.  log-sum-exp as log1p of the sum WITHOUT the maximum's own 1 (a
    // confident graph's loss keeps its relative precision)
    const CandidateChoice ch = candidate_choice(x, Cn, nullptr);
    for (int c = 0; c < Cn; ++c) logits[g * Cn + c] = x[c];
    per_graph[2 * g] = (double)log1pf(ch.rest) + ((double)ch.m - (double)x[0]);    // sparse softmax cross-entropy against class 0 (:425-428)
    per_graph[2 * g + 1] = ch.arg == 0 ? 1.0 : 0.0;
  }
}

// stats = [total_loss, num_correct, total_loss / G, num_correct / G]: thread i adds graphs i, i + 256, ... then a fixed tree
__global__ __launch_bounds__(256) void head_stats_kernel(const double* __restrict__ per_graph, long long G, float* __restrict__ stats) {
  __shared__ double red[4][2];
  double a = 0.0, b = 0.0;
  for (long long g = threadIdx.x; g < G; g += 256) { a += per_graph[2 * g]; b += per_graph[2 * g + 1]; }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = (float)((red[0][0] + red[1][0]) + (red[2][0] + red[3][0]));
    const float correct = (float)((red[0][1] + red[1][1]) + (red[2][1] + red[3][1]));
    stats[0] = total;
    stats[1] = correct;
    stats[2] = total / (float)G;                     // tf.reduce_mean over the graphs (:444); 0 / 0 stays NaN
    stats[3] = correct / (float)G;
  }
}

// Workgroup b walks the graphs b * 4 + wave, + 4 * gridDim.x, ...; every wave writes the rows of ITS graph (zero-filled before) and
// keeps its share of dw in registers; the four waves' shares are added in wave order into the workgroup's partial.
template <int NV>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ H, long long ld, long long V, int D,
                                                       const int* __restrict__ slot_ids, const int* __restrict__ cand_ids,
                                                       const float* __restrict__ mask, const int* __restrict__ first_node,
                                                       long long G, int Cn, const float* __restrict__ w,
                                                       const float* __restrict__ g_loss, const float* __restrict__ g_total,
                                                       float* __restrict__ dH, long long ldg, double* __restrict__ partial) {
  __shared__ double red[4][2 * kHeadMaxD + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float gs = 0.f;
  if (g_loss) gs = g_loss[0] / (float)G;
  if (g_total) gs = g_loss ? gs + g_total[0] : g_total[0];
  double dwc[NV], dws[NV], dwi = 0.0;
#pragma unroll
  for (int q = 0; q < NV; ++q) dwc[q] = dws[q] = 0.0;
  for (long long g = (long long)blockIdx.x * 4 + wave; g < G; g += (long long)gridDim.x * 4) {
    const HeadRows r = head_rows(slot_ids, cand_ids, first_node, g, Cn, V);
    if (!r.ok) continue;                             // (the forward has raised the flag)
    float s[NV], cv[kMaxCn][NV], ip[kMaxCn], x[kMaxCn], gl[kMaxCn];
    head_logits<NV>(H, ld, r, Cn, D, w, mask, g, lane, s, cv, ip, x);
    float m = x[0];
#pragma unroll
    for (int c = 1; c < kMaxCn; ++c) if (c < Cn) m = fmaxf(m, x[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxCn; ++c) { gl[c] = c < Cn ? expf(x[c] - m) : 0.f; sum += gl[c]; }
#pragma unroll
    for (int c = 0; c < kMaxCn; ++c) gl[c] = c < Cn ? gs * (gl[c] / sum - (c == 0 ? 1.f : 0.f)) : 0.f;
    const float wip = w ? w[2 * D] : 1.f;
    float ds[NV], dc[kMaxCn][NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int d = lane + 64 * q;
      const bool in = d < D;
      float acc = 0.f, glsum = 0.f;
#pragma unroll
      for (int c = 0; c < kMaxCn; ++c) {
        const float dip = gl[c] * wip;
        dc[c][q] = dip * s[q] + ((w && in) ? gl[c] * w[d] : 0.f);
        acc += dip * cv[c][q];
        glsum += gl[c];
        dwc[q] += (double)(gl[c] * cv[c][q]);
      }
      ds[q] = acc + ((w && in) ? glsum * w[D + d] : 0.f);
      dws[q] += (double)(glsum * s[q]);
    }
#pragma unroll
    for (int c = 0; c < kMaxCn; ++c) dwi += (double)(gl[c] * ip[c]);
    // rows: candidates in order, then the slot; rows that coincide inside the graph are added in that order and written once
#pragma unroll
    for (int i = 0; i <= kMaxCn; ++i) {
      if (i < kMaxCn && i >= Cn) continue;
      const long long row = i < kMaxCn ? r.cand[i] : r.slot;
      bool seen = false;
#pragma unroll
      for (int j = 0; j < kMaxCn; ++j)
        if (j < i && j < Cn && r.cand[j] == row) seen = true;
      if (seen) continue;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        float v = i < kMaxCn ? dc[i < kMaxCn ? i : 0][q] : ds[q];
#pragma unroll
        for (int j = 1; j < kMaxCn; ++j)
          if (j > i && j < Cn && r.cand[j] == row) v += dc[j][q];
        if (i < kMaxCn && r.slot == row) v += ds[q];
        if (lane + 64 * q < D) dH[row * ldg + lane + 64 * q] = v;
      }
    }
  }
  if (partial == nullptr) return;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    if (lane + 64 * q < D) {
      red[wave][lane + 64 * q] = dwc[q];
      red[wave][D + lane + 64 * q] = dws[q];
    }
  }
  if (lane == 0) red[wave][2 * D] = dwi;
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * D + 1; i += 256)
    partial[(long long)blockIdx.x * (2 * D + 1) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

__global__ __launch_bounds__(256) void head_dw_kernel(const double* __restrict__ partial, int nblk, int n, float* __restrict__ dw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(long long)b * n + i];
  dw[i] = (float)s;
}

static inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

static inline bool charcnn_shape_ok(int32_t C, int32_t D) { return C >= kMinC && C <= kMaxC && D >= 16 && D <= kMaxD && D % 16 == 0; }

static inline long long bwd_labels_per_block(long long U) {
  long long per = (U + kBwdMaxBlocks - 1) / kBwdMaxBlocks;
  per = (per + kBwdTile - 1) / kBwdTile * kBwdTile;
  return per < kBwdRange ? kBwdRange : per;
}

static inline int head_bwd_blocks(long long G) {
  const long long b = (G + 3) / 4;
  return (int)(b < 1 ? 1 : (b > kHeadBlocks ? kHeadBlocks : b));
}

}  // namespace

extern "C" {

int relgnn_charcnn_supported(int32_t num_chars, int32_t out_dim) { return charcnn_shape_ok(num_chars, out_dim) ? 1 : 0; }

int64_t relgnn_charcnn_range_labels(int32_t backward) { return backward ? kBwdRange : kFwdTile; }

size_t relgnn_charcnn_fwd_workspace_bytes(int64_t num_labels, int32_t out_dim, int32_t has_map) {
  if (!has_map || num_labels <= 0 || out_dim <= 0) return 0;
  return align256((size_t)num_labels * out_dim * sizeof(float));
}

int relgnn_charcnn_fwd(const uint8_t* chars, int64_t num_labels, int32_t num_chars, const int32_t* label_of_node, int64_t num_nodes,
                       const float* W1, const float* b1, const float* W2, const float* b2, int32_t out_dim, float* out,
                       void* workspace, size_t workspace_bytes, uint32_t* err_flag, void* stream) {
  if (num_labels < 0 || num_nodes < 0) return RELGNN_EINVAL;
  if (!charcnn_shape_ok(num_chars, out_dim)) return RELGNN_EUNSUPPORTED;
  if (!label_of_node && num_nodes != num_labels) return RELGNN_EINVAL;
  if (num_nodes == 0) return RELGNN_OK;
  if (!W1 || !b1 || !W2 || !b2 || !out || (num_labels > 0 && !chars)) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  float* rep = out;
  if (label_of_node) {
    if (workspace_bytes < relgnn_charcnn_fwd_workspace_bytes(num_labels, out_dim, 1)) return RELGNN_ENOSPC;
    if (num_labels > 0 && !workspace) return RELGNN_EINVAL;
    rep = static_cast<float*>(workspace);
  }
  if (num_labels > 0) {
    const long long ntiles = (num_labels + kFwdTile - 1) / kFwdTile;
    const unsigned grid = (unsigned)(ntiles < 1024 ? ntiles : 1024);
    charcnn_fwd_kernel<<<grid, 256, 0, st>>>(chars, num_labels, num_chars, out_dim, W1, b1, W2, b2, rep);
  }
  if (label_of_node)
    charcnn_gather_kernel<<<flat_grid(num_nodes * out_dim, 256), 256, 0, st>>>(rep, label_of_node, num_nodes, num_labels, out_dim, out,
                                                                              err_flag);
  return launch_status();
}

size_t relgnn_charcnn_bwd_workspace_bytes(int64_t num_labels, int32_t num_chars, int32_t out_dim) {
  if (num_labels <= 0 || !charcnn_shape_ok(num_chars, out_dim)) return 0;
  const int32_t KF = (num_chars - 8) * kF1;
  const long long per = bwd_labels_per_block(num_labels);
  const long long nblk = (num_labels + per - 1) / per;
  return align256((size_t)num_labels * KF * sizeof(float)) + align256((size_t)num_labels * out_dim * sizeof(float)) +
         align256((size_t)nblk * kPartialStride * sizeof(double)) +
         align256((size_t)relgnn_gemm_tn_stream_workspace_bytes(KF, out_dim, num_labels)) +
         align256(relgnn_column_sum_workspace_bytes(num_labels, out_dim));
}

int relgnn_charcnn_bwd(const uint8_t* chars, int64_t num_labels, int32_t num_chars, const float* W1, const float* b1, const float* W2,
                       const float* b2, int32_t out_dim, const float* g_labels, float* dW1, float* db1, float* dW2, float* db2,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (num_labels < 0) return RELGNN_EINVAL;
  if (!charcnn_shape_ok(num_chars, out_dim)) return RELGNN_EUNSUPPORTED;
  if (!W1 || !b1 || !W2 || !b2 || !dW1 || !db1 || !dW2 || !db2) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  const int32_t KF = (num_chars - 8) * kF1;
  if (num_labels == 0) {
    if (hipMemsetAsync(dW1, 0, sizeof(float) * kW1Floats, st) != hipSuccess || hipMemsetAsync(db1, 0, sizeof(float) * kF1, st) != hipSuccess ||
        hipMemsetAsync(dW2, 0, sizeof(float) * KF * out_dim, st) != hipSuccess || hipMemsetAsync(db2, 0, sizeof(float) * out_dim, st) != hipSuccess)
      return RELGNN_EHIP;
    return RELGNN_OK;
  }
  if (!chars || !g_labels || !workspace) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_charcnn_bwd_workspace_bytes(num_labels, num_chars, out_dim)) return RELGNN_ENOSPC;
  const long long per = bwd_labels_per_block(num_labels);
  const int nblk = (int)((num_labels + per - 1) / per);
  char* at = static_cast<char*>(workspace);
  float* P = reinterpret_cast<float*>(at);
  at += align256((size_t)num_labels * KF * sizeof(float));
  float* G2 = reinterpret_cast<float*>(at);
  at += align256((size_t)num_labels * out_dim * sizeof(float));
  double* partial = reinterpret_cast<double*>(at);
  at += align256((size_t)nblk * kPartialStride * sizeof(double));
  void* gemm_ws = at;
  const int64_t gemm_bytes = relgnn_gemm_tn_stream_workspace_bytes(KF, out_dim, num_labels);
  at += align256((size_t)gemm_bytes);
  void* col_ws = at;
  charcnn_bwd_kernel<<<nblk, 256, 0, st>>>(chars, num_labels, num_chars, out_dim, W1, b1, W2, b2, g_labels, P, G2, partial, per);
  charcnn_bwd_combine_kernel<<<(kPartialStride + 255) / 256, 256, 0, st>>>(partial, nblk, dW1, db1);
  int rc = launch_status();
  if (rc != RELGNN_OK) return rc;
  // dW2 [K2 * 16, D] = P^T G2 over the labels: the streaming weight-gradient kernel (chunk partials added in chunk order)
  rc = relgnn_gemm_tn_stream_f32(P, KF, G2, out_dim, dW2, out_dim, KF, out_dim, num_labels, 0, gemm_ws, gemm_bytes, stream);
  if (rc != RELGNN_OK) return rc;
  return relgnn_column_sum(G2, num_labels, out_dim, out_dim, db2, col_ws, relgnn_column_sum_workspace_bytes(num_labels, out_dim), stream);
}

int relgnn_varmisuse_head_supported(int32_t num_candidates, int32_t hidden) {
  return (num_candidates >= 1 && num_candidates <= kMaxCn && hidden >= 64 && hidden <= kHeadMaxD && hidden % 64 == 0) ? 1 : 0;
}

size_t relgnn_varmisuse_head_workspace_bytes(int64_t num_graphs, int32_t hidden) {
  const size_t g = (size_t)(num_graphs > 0 ? num_graphs : 1);
  const size_t fwd = align256(g * 2 * sizeof(double));
  const size_t bwd = align256((size_t)kHeadBlocks * (2 * (size_t)(hidden > 0 ? hidden : 1) + 1) * sizeof(double));
  return fwd > bwd ? fwd : bwd;
}

#define RELGNN_HEAD_DISPATCH(NVC, ...)                                      \
  switch (hidden / 64) {                                                    \
    case 1: { constexpr int NVC = 1; __VA_ARGS__; break; }                  \
    case 2: { constexpr int NVC = 2; __VA_ARGS__; break; }                  \
    case 3: { constexpr int NVC = 3; __VA_ARGS__; break; }                  \
    default: { constexpr int NVC = 4; __VA_ARGS__; break; }                 \
  }

int relgnn_varmisuse_head_fwd(const float* states, int64_t ld, int64_t num_nodes, int32_t hidden, const int32_t* slot_ids,
                              const int32_t* cand_ids, const float* cand_mask, const int32_t* first_node, int64_t num_graphs,
                              int32_t num_candidates, const float* w, float* logits, float* stats, void* workspace,
                              size_t workspace_bytes, uint32_t* err_flag, void* stream) {
  if (num_graphs < 0 || num_nodes < 0 || ld < hidden || !stats) return RELGNN_EINVAL;
  if (!relgnn_varmisuse_head_supported(num_candidates, hidden)) return RELGNN_EUNSUPPORTED;
  if (!workspace || workspace_bytes < relgnn_varmisuse_head_workspace_bytes(num_graphs, hidden)) return RELGNN_ENOSPC;
  if (num_graphs > 0 && (!states || !slot_ids || !cand_ids || !cand_mask || !logits)) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  double* per_graph = static_cast<double*>(workspace);
  if (num_graphs > 0) {
    const unsigned grid = (unsigned)((num_graphs + 3) / 4);
    RELGNN_HEAD_DISPATCH(NVC, head_fwd_kernel<NVC><<<grid, 256, 0, st>>>(states, ld, num_nodes, hidden, slot_ids, cand_ids, cand_mask,
                                                                        first_node, num_graphs, num_candidates, w, logits, per_graph,
                                                                        err_flag));
  }
  head_stats_kernel<<<1, 256, 0, st>>>(per_graph, num_graphs, stats);
  return launch_status();
}

int relgnn_varmisuse_head_bwd(const float* states, int64_t ld, int64_t num_nodes, int32_t hidden, const int32_t* slot_ids,
                              const int32_t* cand_ids, const float* cand_mask, const int32_t* first_node, int64_t num_graphs,
                              int32_t num_candidates, const float* w, const float* g_loss, const float* g_total, float* d_states,
                              int64_t ldg, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
  if (num_graphs < 0 || num_nodes < 0 || ld < hidden || ldg < hidden) return RELGNN_EINVAL;
  if (!relgnn_varmisuse_head_supported(num_candidates, hidden)) return RELGNN_EUNSUPPORTED;
  if ((w != nullptr) != (dw != nullptr)) return RELGNN_EINVAL;
  if (!workspace || workspace_bytes < relgnn_varmisuse_head_workspace_bytes(num_graphs, hidden)) return RELGNN_ENOSPC;
  if (num_nodes > 0 && !d_states) return RELGNN_EINVAL;
  if (num_graphs > 0 && (!states || !slot_ids || !cand_ids || !cand_mask || (!g_loss && !g_total))) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  if (num_nodes > 0 &&
      hipMemset2DAsync(d_states, (size_t)ldg * sizeof(float), 0, (size_t)hidden * sizeof(float), (size_t)num_nodes, st) != hipSuccess)
    return RELGNN_EHIP;
  const int n = 2 * hidden + 1;
  if (num_graphs == 0) {
    if (dw && hipMemsetAsync(dw, 0, sizeof(float) * n, st) != hipSuccess) return RELGNN_EHIP;
    return RELGNN_OK;
  }
  double* partial = dw ? static_cast<double*>(workspace) : nullptr;
  const int nblk = head_bwd_blocks(num_graphs);
  RELGNN_HEAD_DISPATCH(NVC, head_bwd_kernel<NVC><<<nblk, 256, 0, st>>>(states, ld, num_nodes, hidden, slot_ids, cand_ids, cand_mask,
                                                                      first_node, num_graphs, num_candidates, w, g_loss, g_total,
                                                                      d_states, ldg, partial));
  if (dw) head_dw_kernel<<<(n + 255) / 256, 256, 0, st>>>(partial, nblk, n, dw);
  return launch_status();
}

}  // extern "C"
