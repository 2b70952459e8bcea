// The reduction tree of a variable's gradient norm, one definition for relgnn_mt_l2norm (train_utils.hip) and for the norm over
// compact rows (sparse_gradient.hip), which must leave the same bits: per-slot sums of squares in double -> a 64-lane xor butterfly
// -> the four wave sums of a 256-thread block as (r0 + r1) + (r2 + r3) -> kNormChunks block partials -> one more butterfly over the
// partials, padded with +0.0 to 64 lanes -> (float)sqrt.
#pragma once
#include "common.h"

namespace relgnn {

constexpr int kNormChunks = 32;                       // blocks per variable
constexpr int kNormBlock = 256;                       // threads per block: four waves
constexpr int kNormSlots = kNormChunks * kNormBlock;  // element i of a variable belongs to slot i % kNormSlots

__device__ __forceinline__ double norm_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// the block's partial from each thread's slot sum; red: four doubles of LDS.  The value is thread 0's.
__device__ __forceinline__ double norm_block_partial(double acc, double* red) {
  acc = norm_wave_sum(acc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// one wave over the kNormChunks partials of a variable; the value is every lane's
__device__ __forceinline__ float norm_of_partials(const double* __restrict__ partial) {
  const double x = threadIdx.x < kNormChunks ? partial[threadIdx.x] : 0.0;
  return (float)sqrt(norm_wave_sum(x));
}

}  // namespace relgnn
