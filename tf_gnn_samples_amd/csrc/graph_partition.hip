// The wish pass of the device graph partitioner (graph_partition.h states the rule; tasks/graph_partition.py drives the rounds and
// does the admission, the part sizes and the fill phase with integer torch ops).  gfx950 only.
//
// Per eligible node: count the labels of its in-neighbours (all edge types: one contiguous run of col_t), take the lowest label
// among the most frequent ones that differ from the node's own, have room and beat the count of the node's own label.
//   Rows of at most 64 entries: one WAVE per node.  Lane j loads entry j and its source's label; the labels are counted by a
//     ballot match loop: the first live lane's label is broadcast, the lanes that hold it are balloted, counted (popcount) and
//     retired.  One turn per distinct label, at most 64.
//   Longer rows (a hub holds tens of thousands of entries): one WORKGROUP of four waves per node.  A table of P int32 counts in LDS
//     (at most 32 KB), every lane of the workgroup strides over the row and adds 1 to its label's count (integer LDS adds: their
//     order does not change the sum), then every lane scans a stride of the table for its best label, the lanes' bests are merged
//     by a butterfly and the waves' through LDS.  A hub row is spread over 256 lanes, not walked by one wave.
// No global atomics, no float atomics, no spin-wait, no hand-over between workgroups; every loop is bounded by a row length, P or
// a launch argument.  A source outside [0, V) or a label outside [0, P) counts as unassigned (never, for a validated graph and
// the partitioner's own labels): nothing indexes LDS or memory with an unchecked value.
#include "node_set.h"
#include "philox.h"
#include "graph_partition.h"

using namespace relgnn;

namespace {

constexpr int kWaveRowMax = RELGNN_WAVE;     // rows up to here take one wave
constexpr int kMaxParts = 8192;              // the LDS count table: 32 KB
constexpr int kBlock = 256;
constexpr uint32_t kEligibleKey = 0x10000000u;

struct Eligibility {
  const int32_t* anchor;                     // refine: non-zero for the nodes that never move
  int32_t refine;
  uint32_t round, seed;
};

__device__ __forceinline__ bool is_eligible(const Eligibility& e, int32_t v, int32_t own) {
  if (!e.refine) return own < 0;
  if (e.anchor[v] != 0) return false;
  return (philox4x32_10((uint32_t)v, e.round, 0u, 0u, e.seed, kEligibleKey).x & 1u) != 0u;
}

// the label of the source of row entry `entry` of node v: -1 for v itself, an unassigned source and anything out of range
__device__ __forceinline__ int32_t source_label(int32_t entry, int32_t v, int32_t L, int64_t V, int32_t P,
                                                const int32_t* __restrict__ part) {
  const int32_t u = entry / L;
  if (entry < 0 || u == v || (uint32_t)u >= (uint64_t)V) return -1;
  const int32_t label = part[u];
  return (uint32_t)label < (uint32_t)P ? label : -1;
}

// the row of v over all types, or an empty one where rowptr is not what a RelGraph holds
__device__ __forceinline__ void node_row(const int32_t* __restrict__ rowptr, int64_t v, int32_t L, int64_t M, int32_t& b, int32_t& deg) {
  b = rowptr[v * L];
  deg = rowptr[(v + 1) * L] - b;
  if (b < 0 || deg < 0 || (int64_t)b + deg > M) deg = 0;
}

__global__ __launch_bounds__(kBlock) void wish_wave_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                           int32_t L, int64_t M, const int32_t* __restrict__ part,
                                                           const int32_t* __restrict__ room, int32_t P, Eligibility rule,
                                                           int32_t* __restrict__ wish) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (kBlock / RELGNN_WAVE);
  for (int64_t v = blockIdx.x * (int64_t)(kBlock / RELGNN_WAVE) + (threadIdx.x / RELGNN_WAVE); v < V; v += waves) {
    int32_t b, deg;
    node_row(rowptr, v, L, M, b, deg);
    if (deg > kWaveRowMax) continue;                            // the workgroup kernel's (every branch here is the whole wave's)
    const int32_t own = part[v];
    int32_t best = -1;
    if (deg > 0 && is_eligible(rule, (int32_t)v, own)) {
      const int32_t label = lane < deg ? source_label(col[(int64_t)b + lane], (int32_t)v, L, V, P, part) : -1;
      int32_t base = 0, best_count = 0;
      unsigned long long live = __ballot(label >= 0);
      while (live != 0ull) {                                    // one turn per distinct label: `same` holds at least the first lane
        const int32_t l = __shfl(label, __ffsll((long long)live) - 1);
        const unsigned long long same = __ballot(label == l);
        const int32_t c = __popcll(same);
        live &= ~same;
        if (l == own) base = c;
        else if ((c > best_count || (c == best_count && l < best)) && room[l] > 0) { best_count = c; best = l; }
      }
      if (best_count <= base) best = -1;
    }
    if (lane == 0) wish[v] = best;
  }
}

// (count, label) a over b: the larger count, the lower label at equal counts; count 0 is "no label"
__device__ __forceinline__ void take_better(int32_t& count, int32_t& label, int32_t other_count, int32_t other_label) {
  if (other_count > count || (other_count == count && other_count > 0 && other_label < label)) {
    count = other_count;
    label = other_label;
  }
}

__global__ __launch_bounds__(kBlock) void wish_block_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                            int32_t L, int64_t M, const int32_t* __restrict__ part,
                                                            const int32_t* __restrict__ room, int32_t P, Eligibility rule,
                                                            const int32_t* __restrict__ long_nodes,
                                                            const int32_t* __restrict__ long_count, int64_t long_bound,
                                                            int32_t* __restrict__ wish) {
  extern __shared__ int32_t table[];                            // P counts
  __shared__ int32_t wave_count[kBlock / RELGNN_WAVE], wave_label[kBlock / RELGNN_WAVE];
  const int tid = threadIdx.x, lane = tid & (RELGNN_WAVE - 1), wave = tid / RELGNN_WAVE;
  const int64_t n = set_size(long_count, long_bound);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {          // (every branch up to the barriers is the whole workgroup's)
    const int32_t v = long_nodes[i];
    if ((uint32_t)v >= (uint64_t)V) continue;
    const int32_t own = part[v];
    if (!is_eligible(rule, v, own)) {
      if (tid == 0) wish[v] = -1;
      continue;
    }
    int32_t b, deg;
    node_row(rowptr, v, L, M, b, deg);
    for (int32_t l = tid; l < P; l += kBlock) table[l] = 0;
    __syncthreads();
#pragma unroll 4
    for (int32_t j = tid; j < deg; j += kBlock) {
      const int32_t label = source_label(col[(int64_t)b + j], v, L, V, P, part);
      if (label >= 0) atomicAdd(&table[label], 1);
    }
    __syncthreads();
    int32_t best = -1, best_count = 0;
    for (int32_t l = tid; l < P; l += kBlock) {                 // labels ascending per lane: a later equal count does not replace
      const int32_t c = table[l];
      if (c > best_count && l != own && room[l] > 0) { best_count = c; best = l; }
    }
#pragma unroll
    for (int off = RELGNN_WAVE >> 1; off >= 1; off >>= 1) {
      const int32_t oc = __shfl_xor(best_count, off), ol = __shfl_xor(best, off);
      take_better(best_count, best, oc, ol);
    }
    if (lane == 0) { wave_count[wave] = best_count; wave_label[wave] = best; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kBlock / RELGNN_WAVE; ++w) take_better(best_count, best, wave_count[w], wave_label[w]);
      const int32_t base = (uint32_t)own < (uint32_t)P ? table[own] : 0;
      wish[v] = best_count > base ? best : -1;
    }
    __syncthreads();                                            // the table and the waves' bests are the next node's from here
  }
}

}  // namespace

extern "C" {

int relgnn_partition_supported(int64_t num_nodes, int32_t num_edge_types, int64_t num_parts, int32_t imbalance_percent,
                               int32_t refine_rounds) {
  return graph_ok(num_nodes, num_edge_types) && num_parts >= 1 && num_parts <= kMaxParts && num_parts <= num_nodes &&
                 imbalance_percent >= 0 && imbalance_percent <= 100 && refine_rounds >= 0 && refine_rounds <= 64
             ? 1 : 0;
}

int64_t relgnn_partition_wave_row_max(void) { return kWaveRowMax; }

int relgnn_partition_wish(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                          int64_t num_messages, const int32_t* part, const int32_t* room, int32_t num_parts, const int32_t* anchor,
                          int32_t refine, uint32_t round, uint32_t seed, const int32_t* long_nodes, const int32_t* long_count,
                          int64_t long_bound, int32_t classes, int32_t* wish, void* stream) {
  if (num_nodes < 0 || num_messages < 0 || long_bound < 0 || long_bound > num_nodes || classes < 1 || classes > 3) return RELGNN_EINVAL;
  if (num_nodes == 0) return RELGNN_OK;
  if (!relgnn_partition_supported(num_nodes, num_edge_types, num_parts, 0, 0) || num_messages >= ((int64_t)1 << 31) || round > 64u)
    return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !part || !room || !wish || (num_messages > 0 && !col_t) || (refine && !anchor)) return RELGNN_EINVAL;
  if ((classes & 2) && long_bound > 0 && (!long_nodes || !long_count)) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  const Eligibility rule{anchor, refine, round, seed};
  if (classes & 1)
    wish_wave_kernel<<<flat_grid(num_nodes * RELGNN_WAVE, kBlock), kBlock, 0, st>>>(rowptr_t, col_t, num_nodes, num_edge_types,
                                                                                  num_messages, part, room, num_parts, rule, wish);
  if ((classes & 2) && long_bound > 0)
    wish_block_kernel<<<flat_grid(long_bound * kBlock, kBlock), kBlock, (size_t)num_parts * sizeof(int32_t), st>>>(
        rowptr_t, col_t, num_nodes, num_edge_types, num_messages, part, room, num_parts, rule, long_nodes, long_count, long_bound, wish);
  return launch_status();
}

}  // extern "C"
