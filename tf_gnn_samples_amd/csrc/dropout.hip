// tf.nn.dropout on every layer's INPUT (models/sparse_graph_model.py:178-179) and the residual average behind it (:180-185):
//     y = (x / keep_prob) * m,  m in {0.0f, 1.0f}            [TF-internal: div(x, keep_prob) * floor(keep_prob + uniform)]
//     residual layers after the first:  t = y,  cur = (t + last) / 2     (one pass writes both)
// The keep decision of an element is a PURE FUNCTION of (seed, replica, step, stream, flat element index): Philox4x32-10
// (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) with
//     key     = (seed & 0xffffffff, replica)
//     counter = (g lo, g hi, stream, step & 0xffffffff),   g = (element_offset + i) / 4,
// and element i takes output word (element_offset + i) % 4:  keep iff (word >> 8) < T,  T = round(keep_prob * 2^24).
// No mask is stored: the backward regenerates it from the same state block.  seed, replica and step are read from DEVICE
// memory (int64[3]), so a step captured into a hipGraph draws new masks on every replay; nothing the host knows about the step is a
// launch argument.
// True fp32 division and a multiply, not a select: a dropped +-inf / NaN becomes NaN as in the reference (-ffp-contract=off and
// hipcc's correctly rounded fp32 division give the bits of the NumPy composition).
// One thread owns one group of four elements per grid pass (one Philox call): float4 loads / stores when every pointer is
// 16-byte aligned and the group is whole, scalar accesses otherwise (4-byte aligned views, the tail n % 4).  Grid-stride,
// at most 4 blocks of 256 threads per CU of the 256.
// Bound: HBM / Infinity Cache bandwidth, 8 bytes per element (16 for the residual forms): 5.1-5.5 TB/s from 64 MiB to 1 GiB per
// tensor, the rate torch.clone reaches on the same tensors; the Philox rounds hide behind the loads (profiles/layer_dropout.jsonl).
#include "common.h"
#include "philox.h"
#include "../../include/relgnn_dropout.h"

using namespace relgnn;

namespace {

__device__ __forceinline__ float keep_of(uint32_t word, uint32_t T) { return (word >> 8) < T ? 1.0f : 0.0f; }

enum { MODE_DROP = 0, MODE_RES_FWD = 1, MODE_RES_BWD = 2, MODE_RES_BWD_NO_GT = 3 };

// one element.  a / b / o0 / o1 per mode:
//   MODE_DROP          a = x (or gy)               o0 = (a / keep) * m
//   MODE_RES_FWD       a = x, b = last             o0 = t = (a / keep) * m,   o1 = (t + b) / 2
//   MODE_RES_BWD       a = g_cur, b = g_t          o1 = h = a / 2,            o0 = ((b + h) / keep) * m
//   MODE_RES_BWD_NO_GT a = g_cur                   o1 = h = a / 2,            o0 = (h / keep) * m
template <int MODE>
__device__ __forceinline__ void element(float a, float b, float m, float keep, float& o0, float& o1) {
  if constexpr (MODE == MODE_DROP) {
    o0 = (a / keep) * m;
  } else if constexpr (MODE == MODE_RES_FWD) {
    o0 = (a / keep) * m;
    o1 = (o0 + b) / 2.0f;
  } else if constexpr (MODE == MODE_RES_BWD) {
    o1 = a / 2.0f;
    o0 = ((b + o1) / keep) * m;
  } else {
    o1 = a / 2.0f;
    o0 = (o1 / keep) * m;
  }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t n,
                                                      int64_t group_offset, const int64_t* __restrict__ state,
                                                      uint32_t stream_id, uint32_t T, float keep, float* __restrict__ O0,
                                                      float* __restrict__ O1) {
  constexpr bool HAS_B = MODE == MODE_RES_FWD || MODE == MODE_RES_BWD;
  constexpr bool HAS_O1 = MODE != MODE_DROP;
  const uint32_t k0 = (uint32_t)state[0], k1 = (uint32_t)state[1], step = (uint32_t)state[2];
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < groups; j += stride) {
    const uint64_t g = (uint64_t)(group_offset + j);
    const u32x4 r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), stream_id, step, k0, k1);
    const float m0 = keep_of(r.x, T), m1 = keep_of(r.y, T), m2 = keep_of(r.z, T), m3 = keep_of(r.w, T);
    const int64_t i = j << 2;
    if (VEC && i + 4 <= n) {
      const float4 a = *reinterpret_cast<const float4*>(A + i);
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f), o0, o1;
      if constexpr (HAS_B) b = *reinterpret_cast<const float4*>(B + i);
      element<MODE>(a.x, b.x, m0, keep, o0.x, o1.x);
      element<MODE>(a.y, b.y, m1, keep, o0.y, o1.y);
      element<MODE>(a.z, b.z, m2, keep, o0.z, o1.z);
      element<MODE>(a.w, b.w, m3, keep, o0.w, o1.w);
      *reinterpret_cast<float4*>(O0 + i) = o0;
      if constexpr (HAS_O1) *reinterpret_cast<float4*>(O1 + i) = o1;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i + e < n) {
          const float m = e == 0 ? m0 : e == 1 ? m1 : e == 2 ? m2 : m3;
          float b = 0.f, o0, o1;
          if constexpr (HAS_B) b = B[i + e];
          element<MODE>(A[i + e], b, m, keep, o0, o1);
          O0[i + e] = o0;
          if constexpr (HAS_O1) O1[i + e] = o1;
        }
      }
    }
  }
}

inline int check_common(int64_t n, int64_t element_offset, const void* state, int32_t stream_id, uint32_t T, float keep_prob) {
  if (n < 0 || element_offset < 0 || (element_offset & 3) != 0 || stream_id < 0) return RELGNN_EINVAL;
  if (!(keep_prob > 0.f) || !(keep_prob <= 1.f) || T > (1u << 24)) return RELGNN_EINVAL;
  if (n > 0 && !state) return RELGNN_EINVAL;
  if (element_offset > INT64_MAX - n) return RELGNN_EINVAL;
  return RELGNN_OK;
}

template <int MODE>
int launch(const float* A, const float* B, int64_t n, int64_t element_offset, const int64_t* state, int32_t stream_id,
           uint32_t T, float keep_prob, float* O0, float* O1, void* stream) {
  const int64_t groups = (n + 3) >> 2;
  int64_t blocks = (groups + 255) / 256;
  // 4 blocks per CU of the MI355X's 256 (a constant of the one part this library is built for, like flat_grid in common.h:
  // nothing in csrc/ queries the device per launch); the rest by grid stride
  if (blocks > 256 * 4) blocks = 256 * 4;
  const bool vec = aligned16(A) && aligned16(B) && aligned16(O0) && aligned16(O1);      // (NULL counts as aligned)
  if (vec)
    dropout_kernel<MODE, true><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(A, B, n, element_offset >> 2, state,
                                                                               (uint32_t)stream_id, T, keep_prob, O0, O1);
  else
    dropout_kernel<MODE, false><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(A, B, n, element_offset >> 2, state,
                                                                                (uint32_t)stream_id, T, keep_prob, O0, O1);
  return launch_status();
}

}  // namespace

extern "C" {

int relgnn_dropout_fwd(const float* x, int64_t n, int64_t element_offset, const int64_t* state, int32_t stream_id, uint32_t T,
                       float keep_prob, float* y, void* stream) {
  const int st = check_common(n, element_offset, state, stream_id, T, keep_prob);
  if (st != RELGNN_OK) return st;
  if (n == 0) return RELGNN_OK;
  if (!x || !y) return RELGNN_EINVAL;
  return launch<MODE_DROP>(x, nullptr, n, element_offset, state, stream_id, T, keep_prob, y, nullptr, stream);
}

int relgnn_dropout_bwd(const float* gy, int64_t n, int64_t element_offset, const int64_t* state, int32_t stream_id, uint32_t T,
                       float keep_prob, float* gx, void* stream) {
  return relgnn_dropout_fwd(gy, n, element_offset, state, stream_id, T, keep_prob, gx, stream);      // the same map, on gy
}

int relgnn_dropout_residual_fwd(const float* x, const float* last, int64_t n, int64_t element_offset, const int64_t* state,
                                int32_t stream_id, uint32_t T, float keep_prob, float* t, float* cur, void* stream) {
  const int st = check_common(n, element_offset, state, stream_id, T, keep_prob);
  if (st != RELGNN_OK) return st;
  if (n == 0) return RELGNN_OK;
  if (!x || !last || !t || !cur) return RELGNN_EINVAL;
  return launch<MODE_RES_FWD>(x, last, n, element_offset, state, stream_id, T, keep_prob, t, cur, stream);
}

int relgnn_dropout_residual_bwd(const float* g_t, const float* g_cur, int64_t n, int64_t element_offset, const int64_t* state,
                                int32_t stream_id, uint32_t T, float keep_prob, float* g_x, float* g_last, void* stream) {
  const int st = check_common(n, element_offset, state, stream_id, T, keep_prob);
  if (st != RELGNN_OK) return st;
  if (n == 0) return RELGNN_OK;
  if (!g_cur || !g_x || !g_last) return RELGNN_EINVAL;
  if (g_t) return launch<MODE_RES_BWD>(g_cur, g_t, n, element_offset, state, stream_id, T, keep_prob, g_x, g_last, stream);
  return launch<MODE_RES_BWD_NO_GT>(g_cur, nullptr, n, element_offset, state, stream_id, T, keep_prob, g_x, g_last, stream);
}

}  // extern "C"
