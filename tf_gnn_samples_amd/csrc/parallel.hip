// Data-parallel training, the preparation of the ONE gradient all-reduce of a step (parallel.py, PackedGradientAllReducer):
//     flat[off_i + j] = s * grad_i[j]      for every trainable variable i, one behind the other,
// s = float32(w_rank / sum_r w_r).  One launch per RELGNN_MT_MAX variables instead of a multi-tensor copy, a scale, a scalar
// write and a divide behind the collective.  The device pointers ride in the kernel arguments (PackArgs, like MtArgs of
// train_utils.hip): nothing is copied to the device per call, so the launch is capturable.
// Grid (chunks of kQuadsPerBlock * 4 elements, tensors): block (c, t) owns one chunk of tensor t and leaves at once when the
// tensor is shorter (the layout of the fused optimizer updates, which walk the same variable lists).  Within a tensor the
// first 0-3 elements up to the first 16-byte boundary of its DESTINATION slice are scalar (block 0), then whole groups of
// four: one 16-byte store each, fed by one 16-byte load when the source is aligned there too and by four 4-byte loads
// otherwise (a slice behind a variable of odd size, a source that is a view at an odd offset), then a scalar tail.
// The product is __fmul_rn: one rounding, never contracted; a NULL source writes +0.0f (not s * 0).
// Bound: HBM / Infinity Cache bandwidth, 8 bytes per element; the variable sets of the models are 0.1-10 MB, where the
// launch itself is the cost (scripts/bench_dp_pack.py, profiles/dp_train.jsonl).
#include "common.h"
#include "../../include/relgnn_parallel.h"

using namespace relgnn;

namespace {

struct PackArgs {
  const float* g[RELGNN_MT_MAX];
  long long n[RELGNN_MT_MAX];
  long long off[RELGNN_MT_MAX];
};

constexpr int kPackThreads = 256;
constexpr int kQuadsPerBlock = 1024;      // 4096 elements per block: four groups of four per thread

__global__ __launch_bounds__(kPackThreads) void mt_pack_scaled_kernel(PackArgs a, float scale, float* __restrict__ dst) {
  const int t = blockIdx.y;
  const long long n = a.n[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ d = dst + a.off[t];
  // elements in front of the first 16-byte boundary of the destination slice
  long long head = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2;
  if (head > n) head = n;
  const long long quads = (n - head + 3) >> 2;                       // the last one may be partial
  const long long q_beg = (long long)blockIdx.x * kQuadsPerBlock;
  if (blockIdx.x == 0 && (long long)threadIdx.x < head) d[threadIdx.x] = g ? __fmul_rn(g[threadIdx.x], scale) : 0.f;
  if (q_beg >= quads) return;
  const long long q_end = min(quads, q_beg + kQuadsPerBlock);
  const bool vec_load = g && (reinterpret_cast<uintptr_t>(g + head) & 15u) == 0;                   // uniform over the tensor
  for (long long q = q_beg + threadIdx.x; q < q_end; q += kPackThreads) {
    const long long i = head + (q << 2);
    if (i + 4 <= n) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (vec_load) {
        v = *reinterpret_cast<const float4*>(g + i);
      } else if (g) {
        v.x = g[i]; v.y = g[i + 1]; v.z = g[i + 2]; v.w = g[i + 3];
      }
      if (g) {
        v.x = __fmul_rn(v.x, scale); v.y = __fmul_rn(v.y, scale); v.z = __fmul_rn(v.z, scale); v.w = __fmul_rn(v.w, scale);
      }
      *reinterpret_cast<float4*>(d + i) = v;
    } else {
      for (long long e = i; e < n; ++e) d[e] = g ? __fmul_rn(g[e], scale) : 0.f;
    }
  }
}

}  // namespace

extern "C" {

int relgnn_mt_pack_scaled_f32(const float* const* h_grads, const int64_t* h_sizes, int32_t n, float scale, float* dst,
                              void* stream) {
  if (n < 0 || n > RELGNN_MT_MAX) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!h_grads || !h_sizes) return RELGNN_EINVAL;
  PackArgs a;
  long long maxn = 0, off = 0;
  for (int i = 0; i < n; ++i) {
    if (h_sizes[i] < 0 || off > INT64_MAX - h_sizes[i]) return RELGNN_EINVAL;
    if ((reinterpret_cast<uintptr_t>(h_grads[i]) & 3u) != 0) return RELGNN_EINVAL;
    a.g[i] = h_grads[i];
    a.n[i] = h_sizes[i];
    a.off[i] = off;
    off += h_sizes[i];
    if (h_sizes[i] > maxn) maxn = h_sizes[i];
  }
  if (maxn == 0) return RELGNN_OK;
  if (!dst || (reinterpret_cast<uintptr_t>(dst) & 3u) != 0) return RELGNN_EINVAL;
  const long long per_block = (long long)kQuadsPerBlock * 4;
  const long long chunks = (maxn + per_block - 1) / per_block;
  if (chunks > 0x7fffffffLL) return RELGNN_EINVAL;
  mt_pack_scaled_kernel<<<dim3((unsigned)chunks, (unsigned)n), kPackThreads, 0, as_stream(stream)>>>(a, scale, dst);
  return launch_status();
}

}  // extern "C"
