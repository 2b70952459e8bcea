// The stamped node set under both device samplers (neighbour_sample.hip, subgraph_sample.hip; StampedNodeSet of
// tasks/neighbour_sampling.py holds the array): the pieces the two files share.  gfx950 only.
//
// A sampler keeps ONE [V] int32 stamp array per graph, all zero between calls and after a call that raised (the Python side zeroes
// the whole array then).  A call stamps a node set, compacts it into an ascending list (relgnn_neighbour_sample_compact, a flag scan
// over the stamps: the compaction belongs to the node set, the entry point keeps the name it was exported under), counts the bucket
// entries per (node, type), scans the counts into offsets, reads the sizes back once, emits edges and clears the listed stamps.  A stamp:
//   neighbour sampling   -1: a seed;  h + 1: first reached by hop h = 0, 1, ... (the node's distance from the seeds).
//   subgraph sampling    1: visited by a walk (-1: named by the caller, relgnn_neighbour_sample_begin);  once the set is listed,
//                        position + 1 (relgnn_subgraph_number): a source's local id is its stamp - 1.
// No atomics: a stamp is written with a plain store of the one value every writer of that launch writes.
#pragma once
#include "common.h"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace relgnn {
namespace {      // (every translation unit that includes this gets its own copy, of the kernel too)

inline bool graph_ok(int64_t V, int32_t L) { return V > 0 && L > 0 && V * (int64_t)L < ((int64_t)1 << 31); }

// a size that is still on the device (a frontier's or a node list's length), clamped to the bound its buffers were sized from
__device__ __forceinline__ int64_t set_size(const int32_t* __restrict__ count, int64_t bound) {
  const int64_t n = *count;
  return n < 0 ? 0 : (n > bound ? bound : n);
}

// what a compaction keeps: the stamps equal to `value`, every non-zero stamp when value == 0
struct StampFlag {
  int32_t value;
  __device__ __forceinline__ int32_t operator()(int32_t s) const { return (value != 0 ? s == value : s != 0) ? 1 : 0; }
};

// offsets = the exclusive sums of counts[l * B + i] and a closing entry -> totals[l] = the entries of type l, totals[L] = all
__global__ __launch_bounds__(64) void bucket_totals_kernel(const int32_t* __restrict__ offsets, int64_t B, int32_t L,
                                                          int32_t* __restrict__ totals) {
  for (int32_t l = threadIdx.x; l <= L; l += blockDim.x)
    totals[l] = l < L ? offsets[(int64_t)(l + 1) * B] - offsets[(int64_t)l * B] : offsets[(int64_t)L * B];
}

// rocPRIM's storage for an exclusive scan of `items` int32; kWithFlagged: the larger of that and the compaction's scan over StampFlag's
// transform iterator, for a workspace that serves both (a template argument: a file that compacts nothing compiles no flagged scan)
template <bool kWithFlagged>
inline size_t scan_temp_bytes(int64_t items) {
  size_t plain = 0, flagged = 0;
  int32_t* p = nullptr;
  rocprim::exclusive_scan(nullptr, plain, p, p, (int32_t)0, (size_t)items, rocprim::plus<int32_t>(), (hipStream_t)0);
  if constexpr (kWithFlagged) {
    auto flags = rocprim::make_transform_iterator(static_cast<const int32_t*>(nullptr), StampFlag{0});
    rocprim::exclusive_scan(nullptr, flagged, flags, p, (int32_t)0, (size_t)items, rocprim::plus<int32_t>(), (hipStream_t)0);
  }
  return plain > flagged ? plain : flagged;
}

// behind a sampler's own count kernel: counts[0 .. B * L] -> offsets (rocPRIM's scan, in `temp` of the caller's workspace) -> totals
inline int scan_bucket_counts(int32_t* counts, int32_t* offsets, int64_t B, int32_t L, int32_t* totals, void* temp, size_t temp_bytes,
                              hipStream_t st) {
  if (rocprim::exclusive_scan(temp, temp_bytes, counts, offsets, (int32_t)0, (size_t)(B * L + 1), rocprim::plus<int32_t>(), st) != hipSuccess)
    return RELGNN_EHIP;
  bucket_totals_kernel<<<1, 64, 0, st>>>(offsets, B, L, totals);
  return launch_status();
}

}  // namespace
}  // namespace relgnn
