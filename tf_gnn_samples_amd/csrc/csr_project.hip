// CSR rows times a dense row table: the input projection of sparse node features, and (over the transposed structure, with the
// activation gradient folded into the gathered rows) its weight gradient.  include/relgnn_sparse_features.h states the contract
// and the summation order.
//
// The kernel is the gather of seg_reduce.hip with the rows coming from the weight matrix and a scale per entry:
//   * a wave owns an output row, a lane four consecutive columns (one 16-byte load; 64 lanes = 1 KiB); for n > 256 the lane walks
//     the column groups one after the other (the index stream of a row is re-read from cache, the table rows are not);
//   * the column ids and values of up to 64 entries are fetched with one coalesced load each and broadcast with v_readlane into
//     SGPRs: every row load is `scalar base + lane offset`;
//   * kUnroll independent row loads are in flight before the first add, in straight-line code: a load under a condition makes hipcc
//     drain the pipeline (seg_reduce.hip).  The tail of a batch gathers the batch's first entry again under a
//     scale of +0; lanes behind the row's width read a clamped column and store nothing.
//   * rows of more than kSplitAbove entries go to a workgroup per slab of kSlab entries (four waves, partial sums combined through
//     LDS in wave order) and, where a row has several slabs, a second pass over the slab sums in ascending order.
// Bound: HBM / Infinity-Cache bandwidth.  Algorithmic bytes per launch: nnz * (4 n + 8) [+ nnz * 4 n for y] + rows * 4 n.
#include "common.h"

#include "../../include/relgnn_sparse_features.h"

using namespace relgnn;

namespace {

constexpr int kUnroll = 8;
constexpr int kSplitAbove = 128;   // rows longer than this are split
constexpr int kWaveShare = 128;    // entries of a slab one wave sums
constexpr int kSlab = 4 * kWaveShare;

__device__ __forceinline__ float epilogue(int act, float x) {
  switch (act) {
    case RELGNN_ACT_TANH: return act_fwd<RELGNN_ACT_TANH>(x);
    case RELGNN_ACT_RELU: return act_fwd<RELGNN_ACT_RELU>(x);
    case RELGNN_ACT_LEAKY_RELU: return act_fwd<RELGNN_ACT_LEAKY_RELU>(x);
    case RELGNN_ACT_ELU: return act_fwd<RELGNN_ACT_ELU>(x);
    case RELGNN_ACT_SELU: return act_fwd<RELGNN_ACT_SELU>(x);
    case RELGNN_ACT_GELU: return act_fwd<RELGNN_ACT_GELU>(x);
    default: return x;
  }
}

__device__ __forceinline__ float4 epilogue4(int act, float4 a) {
  if (act != RELGNN_ACT_LINEAR) {
    a.x = epilogue(act, a.x); a.y = epilogue(act, a.y); a.z = epilogue(act, a.z); a.w = epilogue(act, a.w);
  }
  return a;
}

// acc += s * (t [* act'(y)]): every product and the add rounded on its own (-ffp-contract=off)
template <int DACT>
__device__ __forceinline__ void add_term(float4& acc, float s, float4 t, const float4& yy) {
  if constexpr (DACT != RELGNN_ACT_LINEAR) {
    t.x *= dact_from_output(DACT, yy.x); t.y *= dact_from_output(DACT, yy.y);
    t.z *= dact_from_output(DACT, yy.z); t.w *= dact_from_output(DACT, yy.w);
  }
  const float4 m = make_float4(s * t.x, s * t.y, s * t.z, s * t.w);
  acc.x += m.x; acc.y += m.y; acc.z += m.z; acc.w += m.w;
}

// The sum of entries [beg, end) (wave-uniform) for this lane's four columns, ascending, starting from +0.
// c4: the lane's float4 column, clamped into the row.  DACT != LINEAR: the gradient form, y gathered beside the table.
template <int DACT>
__device__ __forceinline__ float4 sum_entries(int beg, int end, const int32_t* __restrict__ col, const float* __restrict__ val,
                                              const float4* __restrict__ table, int64_t ldt4, const float4* __restrict__ y,
                                              int64_t ldy4, int c4, int lane) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; p += 64) {
    const int nb = min(64, end - p);
    // one coalesced load of ids and one of values per 64 entries; lanes behind the batch repeat its first entry under a scale of 0
    const int at = p + (lane < nb ? lane : 0);
    const int my_col = col[at];
    const float loaded = val[at];
    const float my_val = lane < nb ? loaded : 0.f;
    for (int k = 0; k < nb; k += kUnroll) {      // k + u <= 63: nb <= 64 and k is a multiple of kUnroll
      float4 t[kUnroll], yy[DACT != RELGNN_ACT_LINEAR ? kUnroll : 1];
      float s[kUnroll];
      if constexpr (DACT == RELGNN_ACT_LINEAR) yy[0] = make_float4(0.f, 0.f, 0.f, 0.f);      // (never read)
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t r = (int64_t)__builtin_amdgcn_readlane(my_col, k + u);
        s[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_val), k + u));
        t[u] = (table + r * ldt4)[c4];           // scalar (SGPR) row base
        if constexpr (DACT != RELGNN_ACT_LINEAR) yy[u] = (y + r * ldy4)[c4];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) add_term<DACT>(acc, s[u], t[u], yy[DACT != RELGNN_ACT_LINEAR ? u : 0]);
    }
  }
  return acc;
}

// ---- one wave per row; rows longer than split_above are left to the slab kernel ------------------------------------------------
template <int DACT>
__global__ __launch_bounds__(256) void csr_project_rows_kernel(
    const int32_t* __restrict__ rowptr, int64_t num_rows, const int32_t* __restrict__ col, const float* __restrict__ val,
    const float4* __restrict__ table, int64_t ldt4, const float4* __restrict__ y, int64_t ldy4, int32_t n4, int32_t act,
    int32_t split_above, float4* __restrict__ out, int64_t ldo4) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= num_rows) return;
  const int beg = __builtin_amdgcn_readfirstlane(rowptr[r]);
  const int end = __builtin_amdgcn_readfirstlane(rowptr[r + 1]);
  if (end - beg > split_above) return;
  for (int g = 0; g < n4; g += 64) {
    const int c = g + lane;
    const float4 acc = sum_entries<DACT>(beg, end, col, val, table, ldt4, y, ldy4, min(c, n4 - 1), lane);
    if (c < n4) out[r * ldo4 + c] = epilogue4(DACT == RELGNN_ACT_LINEAR ? act : RELGNN_ACT_LINEAR, acc);
  }
}

// ---- one workgroup per slab of a long row ---------------------------------------------------------------------------------------
template <int DACT>
__global__ __launch_bounds__(256) void csr_project_slabs_kernel(
    const int32_t* __restrict__ slabs, const int32_t* __restrict__ col, const float* __restrict__ val,
    const float4* __restrict__ table, int64_t ldt4, const float4* __restrict__ y, int64_t ldy4, int32_t n4, int32_t act,
    float4* __restrict__ ws, float4* __restrict__ out, int64_t ldo4) {
  __shared__ float4 part[3][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int32_t* slab = slabs + (int64_t)blockIdx.x * 4;
  const int64_t row = slab[0];
  const int sbeg = slab[1], send = slab[2], dest = slab[3];
  const int beg = min(sbeg + w * kWaveShare, send);
  const int end = min(beg + kWaveShare, send);
  for (int g = 0; g < n4; g += 64) {
    const int c = g + lane;
    float4 acc = sum_entries<DACT>(beg, end, col, val, table, ldt4, y, ldy4, min(c, n4 - 1), lane);
    if (g) __syncthreads();                       // the previous column group's partial sums have been read
    if (w) part[w - 1][lane] = acc;
    __syncthreads();
    if (w == 0 && c < n4) {
#pragma unroll
      for (int o = 0; o < 3; ++o) {               // ((p0 + p1) + p2) + p3
        const float4 p = part[o][lane];
        acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
      }
      if (dest < 0) out[row * ldo4 + c] = epilogue4(DACT == RELGNN_ACT_LINEAR ? act : RELGNN_ACT_LINEAR, acc);
      else ws[(int64_t)dest * n4 + c] = acc;
    }
  }
}

// ---- rows of several slabs: the slab sums in ascending order, one wave per row ----------------------------------------------------
__global__ __launch_bounds__(256) void csr_project_combine_kernel(const int32_t* __restrict__ combos, int64_t num_combos,
                                                                  const float4* __restrict__ ws, int32_t n4, int32_t act,
                                                                  float4* __restrict__ out, int64_t ldo4) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= num_combos) return;
  const int64_t row = combos[3 * i];
  const int64_t first = combos[3 * i + 1];
  const int count = __builtin_amdgcn_readfirstlane(combos[3 * i + 2]);
  for (int c = lane; c < n4; c += 64) {
    const float4* src = ws + first * n4 + c;
    float4 acc = src[0];
    for (int s = 1; s < count; ++s) {
      const float4 p = src[(int64_t)s * n4];
      acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
    }
    out[row * ldo4 + c] = epilogue4(act, acc);
  }
}

template <int DACT>
int launch_all(int32_t act, const int32_t* rowptr, int64_t num_rows, const int32_t* col, const float* val, const float* table,
               int64_t ld_table, const float* y, int64_t ld_y, int32_t n, const int32_t* slabs, int64_t num_slabs,
               const int32_t* combos, int64_t num_combos, float* ws, float* out, int64_t ld_out, hipStream_t stream) {
  const float4* t4 = reinterpret_cast<const float4*>(table);
  const float4* y4 = reinterpret_cast<const float4*>(y);
  float4* o4 = reinterpret_cast<float4*>(out);
  const int32_t n4 = n / 4;
  const int32_t split_above = num_slabs > 0 ? kSplitAbove : INT32_MAX;
  csr_project_rows_kernel<DACT><<<dim3((unsigned)((num_rows + 3) / 4)), dim3(256), 0, stream>>>(
      rowptr, num_rows, col, val, t4, ld_table / 4, y4, ld_y / 4, n4, act, split_above, o4, ld_out / 4);
  int st = launch_status();
  if (st != RELGNN_OK || num_slabs == 0) return st;
  csr_project_slabs_kernel<DACT><<<dim3((unsigned)num_slabs), dim3(256), 0, stream>>>(
      slabs, col, val, t4, ld_table / 4, y4, ld_y / 4, n4, act, reinterpret_cast<float4*>(ws), o4, ld_out / 4);
  st = launch_status();
  if (st != RELGNN_OK || num_combos == 0) return st;
  csr_project_combine_kernel<<<dim3((unsigned)((num_combos + 3) / 4)), dim3(256), 0, stream>>>(
      combos, num_combos, reinterpret_cast<const float4*>(ws), n4, DACT == RELGNN_ACT_LINEAR ? act : RELGNN_ACT_LINEAR, o4,
      ld_out / 4);
  return launch_status();
}

}  // namespace

extern "C" {

int relgnn_csr_project_supported(int32_t n) { return n >= 4 && n <= 1024 && n % 4 == 0; }
int64_t relgnn_csr_project_split_above(void) { return kSplitAbove; }
int64_t relgnn_csr_project_slab(void) { return kSlab; }

int relgnn_csr_project_f32(int32_t act, const int32_t* rowptr, int64_t num_rows, const int32_t* col, const float* val,
                           int64_t nnz, const float* table, int64_t table_rows, int64_t ld_table, const float* y,
                           int64_t ld_y, int32_t n, const int32_t* slabs, int64_t num_slabs, const int32_t* combos,
                           int64_t num_combos, float* ws, int64_t ws_rows, float* out, int64_t ld_out, void* stream) {
  if (num_rows < 0 || nnz < 0 || table_rows < 0 || num_slabs < 0 || num_combos < 0 || ws_rows < 0) return RELGNN_EINVAL;
  if (nnz >= INT32_MAX || num_rows >= INT32_MAX || num_slabs >= INT32_MAX || ws_rows >= INT32_MAX) return RELGNN_EINVAL;
  if (act < RELGNN_ACT_LINEAR || act > RELGNN_ACT_GELU || (y && act == RELGNN_ACT_GELU)) return RELGNN_EINVAL;
  if (!relgnn_csr_project_supported(n)) return RELGNN_EUNSUPPORTED;
  if (num_rows == 0) return RELGNN_OK;
  if (!rowptr || !out || (nnz > 0 && (!col || !val || !table || table_rows == 0))) return RELGNN_EINVAL;
  if (ld_out < n || ld_out % 4 || !aligned16(out)) return RELGNN_EINVAL;
  if (nnz > 0 && (ld_table < n || ld_table % 4 || !aligned16(table))) return RELGNN_EINVAL;
  if (y && nnz > 0 && (ld_y < n || ld_y % 4 || !aligned16(y))) return RELGNN_EINVAL;
  if (num_slabs > 0 && !slabs) return RELGNN_EINVAL;
  if (num_combos > 0 && (!combos || !ws || !aligned16(ws) || num_slabs == 0)) return RELGNN_EINVAL;
  const hipStream_t s = as_stream(stream);
#define RELGNN_CSR_LAUNCH(DACT)                                                                                              \
  return launch_all<DACT>(act, rowptr, num_rows, col, val, table, ld_table, y, ld_y, n, slabs, num_slabs, combos, num_combos, \
                          ws, out, ld_out, s)
  if (!y || act == RELGNN_ACT_LINEAR) {
    // (a linear gradient gathers no y: dact is 1)
    if (y) act = RELGNN_ACT_LINEAR;
    RELGNN_CSR_LAUNCH(RELGNN_ACT_LINEAR);
  }
  switch (act) {
    case RELGNN_ACT_TANH: RELGNN_CSR_LAUNCH(RELGNN_ACT_TANH);
    case RELGNN_ACT_RELU: RELGNN_CSR_LAUNCH(RELGNN_ACT_RELU);
    case RELGNN_ACT_LEAKY_RELU: RELGNN_CSR_LAUNCH(RELGNN_ACT_LEAKY_RELU);
    case RELGNN_ACT_ELU: RELGNN_CSR_LAUNCH(RELGNN_ACT_ELU);
    case RELGNN_ACT_SELU: RELGNN_CSR_LAUNCH(RELGNN_ACT_SELU);
    default: return RELGNN_EINVAL;
  }
#undef RELGNN_CSR_LAUNCH
}

}  // extern "C"
