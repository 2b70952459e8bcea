// The compact gradient of a [F, n] row table (include/relgnn_sparse_gradient.h): which words a batch's transposed structure names
// (tasks/sparse_features.py SparseRows.named_rows drives the two steps) and the dense clip norm's bits from the named rows alone.
// The row step on compact rows lives with its dense sibling in sparse_update.hip.
//
// Named rows: slot = an exclusive scan of "row f has entries", read through a transform iterator (no flag array); one thread hands T
// to the caller's read-back buffer; the fill is one grid-stride kernel of three independent loops (words and rowptr_c per word, the
// remapped slabs, the remapped combos).  Every store is checked against a capacity; no atomics; no hand-over between workgroups.
//
// Norm: relgnn_mt_l2norm gives element i of the dense gradient to slot i % 8192 and adds a slot's squares in ascending i.  Here block b
// owns slots [256 b, 256 b + 256) as there; it reads `words` in tiles of 1024, keeps in LDS — in order — the rows whose n elements meet
// its slots (a test on (word * n) % 8192 that is the same for every thread of the block), and each thread then adds, row after row,
// the one element of the row that falls on its slot, or +0.0 (which leaves a non-negative sum as it is).  For a width that divides
// 8192 a row meets one block (n <= 256) or n / 256 whole blocks; otherwise rows straddle blocks and the per-thread test decides.
// The tree behind the slot sums is norm_tree.h's, the one relgnn_mt_l2norm compiles.
#include "common.h"
#include "norm_tree.h"
#include "../../include/relgnn_sparse_gradient.h"
#include "../../include/relgnn_sparse_update.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

using namespace relgnn;

namespace {

constexpr int64_t kIndexLimit = INT32_MAX;

// item f of the scan: 1 when word f has entries; the closing item (f == F) is 0
struct NamedFlag {
  const int32_t* rowptr;
  int64_t F;
  __device__ __forceinline__ int32_t operator()(int64_t f) const { return f < F && rowptr[f + 1] > rowptr[f] ? 1 : 0; }
};

size_t named_scan_temp_bytes(int64_t items) {
  size_t bytes = 0;
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), NamedFlag{nullptr, 0});
  rocprim::exclusive_scan(nullptr, bytes, in, static_cast<int32_t*>(nullptr), (int32_t)0, (size_t)items, rocprim::plus<int32_t>(),
                          (hipStream_t)0);
  return bytes;
}

__global__ __launch_bounds__(64) void named_count_kernel(const int32_t* __restrict__ total, int32_t* __restrict__ count) {
  if (threadIdx.x == 0) *count = *total;
}

__global__ __launch_bounds__(256) void named_fill_kernel(const int32_t* __restrict__ rowptr_t, int64_t F,
                                                         const int32_t* __restrict__ slot, int64_t T, int32_t* __restrict__ words,
                                                         int32_t* __restrict__ rowptr_c, const int4* __restrict__ slabs_t,
                                                         int4* __restrict__ slabs_c, int64_t num_slabs,
                                                         const int32_t* __restrict__ combos_t, int32_t* __restrict__ combos_c,
                                                         int64_t num_combos) {
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t f = first; f <= F; f += stride) {
    if (f == F) {
      rowptr_c[T] = rowptr_t[F];                              // (the array has T + 1 entries)
      continue;
    }
    const int32_t begin = rowptr_t[f];
    if (rowptr_t[f + 1] <= begin) continue;
    const int64_t t = slot[f];
    if (t < 0 || t >= T) continue;
    words[t] = (int32_t)f;
    rowptr_c[t] = begin;
  }
  // the slot of a plan row; -1 for what no plan of this structure holds
  auto slot_of = [&](int32_t row) -> int32_t {
    if (row < 0 || row >= F) return -1;
    const int32_t t = slot[row];
    return t >= 0 && t < T ? t : -1;
  };
  for (int64_t s = first; s < num_slabs; s += stride) {
    int4 slab = slabs_t[s];
    const int32_t t = slot_of(slab.x);
    slabs_c[s] = t >= 0 ? make_int4(t, slab.y, slab.z, slab.w) : make_int4(0, 0, 0, -1);
  }
  for (int64_t c = first; c < num_combos; c += stride) {
    const int32_t t = slot_of(combos_t[c * 3]);
    combos_c[c * 3] = t >= 0 ? t : 0;
    combos_c[c * 3 + 1] = t >= 0 ? combos_t[c * 3 + 1] : 0;
    combos_c[c * 3 + 2] = t >= 0 ? combos_t[c * 3 + 2] : 0;
  }
}

constexpr int kTile = 4 * kNormBlock;       // words a block looks at between two barriers

__global__ __launch_bounds__(kNormBlock) void rows_l2norm_partial_kernel(const int32_t* __restrict__ words, long long T,
                                                                         const float* __restrict__ g, long long ld_g, int n,
                                                                         long long F, double* __restrict__ partial) {
  __shared__ double red[4];
  __shared__ int32_t list_row[kTile];         // tile-relative compact row of a kept row, in ascending order
  __shared__ uint32_t list_start[kTile];      // (word * n) % 8192: the slot of its element 0
  __shared__ int counts[4][4];                // [pass][wave]: rows kept
  const uint32_t mask = kNormSlots - 1;
  const uint32_t block_slot = blockIdx.x * kNormBlock, my_slot = block_slot + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  double acc = 0.0;
  for (long long base = 0; base < T; base += kTile) {
    bool keep[4];
    uint32_t start[4];
    int within[4];
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const long long t = base + pass * kNormBlock + threadIdx.x;
      keep[pass] = false;
      start[pass] = 0;
      if (t < T) {
        const long long f = words[t];
        if (f >= 0 && f < F) {
          start[pass] = ((uint32_t)f * (uint32_t)n) & mask;        // (2^32 is a multiple of 8192: the wrap is harmless)
          // the row holds the block's first slot, or the block holds the row's first
          keep[pass] = ((block_slot - start[pass]) & mask) < (uint32_t)n || ((start[pass] - block_slot) & mask) < (uint32_t)kNormBlock;
        }
      }
      const unsigned long long kept = __ballot(keep[pass]);
      within[pass] = __popcll(kept & below);
      if (lane == 0) counts[pass][wave] = __popcll(kept);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w == wave && keep[pass]) {
          list_row[total + within[pass]] = pass * kNormBlock + threadIdx.x;
          list_start[total + within[pass]] = start[pass];
        }
        total += counts[pass][w];
      }
    }
    __syncthreads();
    const float* __restrict__ tile = g + base * ld_g;
#pragma unroll 4
    for (int j = 0; j < total; ++j) {                             // total <= kTile
      const uint32_t c = (my_slot - list_start[j]) & mask;
      const bool mine = c < (uint32_t)n;
      const double x = tile[(long long)list_row[j] * ld_g + (mine ? c : 0u)];
      acc += mine ? x * x : 0.0;                                  // (+0.0 leaves a sum of squares as it is, NaN and inf included)
    }
    __syncthreads();                                              // the lists are rewritten by the next tile
  }
  const double sum = norm_block_partial(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void rows_l2norm_final_kernel(const double* __restrict__ partial, float* __restrict__ norm) {
  const float value = norm_of_partials(partial);
  if (threadIdx.x == 0) norm[0] = value;
}

}  // namespace

extern "C" {

size_t relgnn_named_rows_workspace_bytes(int64_t F) {
  if (F < 0) F = 0;
  return align_up(named_scan_temp_bytes(F + 1), 256) + 256;
}

int relgnn_named_rows_count(const int32_t* rowptr_t, int64_t F, int32_t* slot, int32_t* count, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (F < 0 || !rowptr_t || !slot || !count || !workspace) return RELGNN_EINVAL;
  if (F >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (workspace_bytes < relgnn_named_rows_workspace_bytes(F)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), NamedFlag{rowptr_t, F});
  size_t bytes = workspace_bytes;
  if (rocprim::exclusive_scan(workspace, bytes, in, slot, (int32_t)0, (size_t)(F + 1), rocprim::plus<int32_t>(), st) != hipSuccess)
    return RELGNN_EHIP;
  named_count_kernel<<<1, 64, 0, st>>>(slot + F, count);
  return launch_status();
}

int relgnn_named_rows_fill(const int32_t* rowptr_t, int64_t F, const int32_t* slot, int64_t T, int32_t* words,
                           int32_t* rowptr_c, const int32_t* slabs_t, int32_t* slabs_c, int64_t num_slabs,
                           const int32_t* combos_t, int32_t* combos_c, int64_t num_combos, void* stream) {
  if (F < 0 || T < 0 || T > F || num_slabs < 0 || num_combos < 0) return RELGNN_EINVAL;
  if (F >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (T == 0) return RELGNN_OK;
  if (!rowptr_t || !slot || !words || !rowptr_c) return RELGNN_EINVAL;
  if (num_slabs > 0 && (!slabs_t || !slabs_c || !aligned16(slabs_t) || !aligned16(slabs_c))) return RELGNN_EINVAL;
  if (num_combos > 0 && (!combos_t || !combos_c)) return RELGNN_EINVAL;
  const int64_t items = F + 1 > num_slabs ? F + 1 : num_slabs;            // (combos <= slabs)
  named_fill_kernel<<<flat_grid(items > num_combos ? items : num_combos, 256), 256, 0, as_stream(stream)>>>(
      rowptr_t, F, slot, T, words, rowptr_c, reinterpret_cast<const int4*>(slabs_t), reinterpret_cast<int4*>(slabs_c), num_slabs,
      combos_t, combos_c, num_combos);
  return launch_status();
}

size_t relgnn_rows_l2norm_workspace_bytes(void) { return (size_t)kNormChunks * sizeof(double); }

int relgnn_rows_l2norm(const int32_t* words, int64_t T, const float* g, int64_t ld_g, int32_t n, int64_t F, float* norm,
                       void* workspace, size_t workspace_bytes, void* stream) {
  if (T < 0 || F < 0 || T > F || !norm) return RELGNN_EINVAL;
  if (F >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (!relgnn_rows_adam_supported(n)) return RELGNN_EUNSUPPORTED;
  if (T > 0 && (!words || !g || ld_g < n)) return RELGNN_EINVAL;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_rows_l2norm_workspace_bytes()) return RELGNN_ENOSPC;
  double* partial = static_cast<double*>(workspace);
  rows_l2norm_partial_kernel<<<kNormChunks, kNormBlock, 0, as_stream(stream)>>>(words, T, g, ld_g, n, F, partial);
  rows_l2norm_final_kernel<<<1, 64, 0, as_stream(stream)>>>(partial, norm);
  return launch_status();
}

}  // extern "C"
