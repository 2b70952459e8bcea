// Neighbour sampling for single-graph node classification (include/relgnn_sampling.h states the rule; tasks/neighbour_sampling.py
// drives the hops): a fanout-limited neighbourhood of a seed list, drawn from the by-target bucketing of the full graph in place.
//
// One WAVE owns one (frontier node, edge type) bucket.  A bucket of at most k entries (or any bucket when k == 0) is copied.  A
// longer one, of any length, is sampled without LDS and without per-lane arrays: lane q walks the positions q, q + 64, ... and keeps
// the smallest key (word_j << 32 | j) it has not given away yet; k rounds of a wave-wide arg-min (six xor shuffles of a 64-bit key)
// take the k smallest keys of the bucket.  A lane keeps its THREE smallest keys from one walk over its positions; the lane that owned
// a round's winner moves on to its next one, and only a lane that wins a third time walks its positions again, for its smallest keys
// above the one just taken (a lane's keys leave in ascending order, so "above the last one taken" is "not yet taken").
// Lane r keeps the position taken in round r; the ranks of the k positions among themselves (k shuffles) give the output slots, so
// the entries come out in ascending position.  Work per bucket: deg / 64 Philox calls per lane, and one more such walk per third
// win of a lane: rare for a long bucket (k wins spread over 64 lanes), at most k / 3 walks.  Every loop is bounded by deg, k, or a
// launch argument.
// The hop's offsets come from min(deg, k) alone (rocPRIM's device scan, the library plan.hip sorts with), so nothing counts sampled
// edges, and new nodes are found by a flag scan over the stamps.  No atomics anywhere: a stamp is written with a plain store of the
// one value every writer of the hop writes.
// What the stamps mean, the clamped device count and the scan of a hop's counts into offsets and totals are node_set.h's, shared with
// subgraph_sample.hip; the compaction of the stamped set (relgnn_neighbour_sample_compact) is defined here and serves both samplers.
#include "node_set.h"
#include "philox.h"
#include "../../include/relgnn_sampling.h"
#include "../../include/relgnn_layered_sampling.h"

using namespace relgnn;

namespace {

constexpr int kMaxFanout = 64;
constexpr int kMaxHops = 8;
constexpr int32_t kSeedStamp = -1;

__global__ __launch_bounds__(256) void begin_kernel(const int32_t* __restrict__ seeds, int64_t num_seeds, int32_t* __restrict__ stamp,
                                                    int64_t V) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < num_seeds; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t s = seeds[i];
    if ((uint32_t)s < (uint64_t)V) stamp[s] = kSeedStamp;
  }
}

// counts[l * B + i] = min(deg, k) (deg where k == 0), 0 beyond the frontier and in the closing entry
__global__ __launch_bounds__(256) void count_kernel(const int32_t* __restrict__ rowptr, int32_t L, const int32_t* __restrict__ frontier,
                                                    const int32_t* __restrict__ frontier_count, int64_t B, int32_t k,
                                                    int32_t* __restrict__ counts) {
  const int64_t nf = set_size(frontier_count, B), total = B * L;
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w <= total; w += (int64_t)gridDim.x * blockDim.x) {
    int32_t c = 0;
    if (w < total) {
      const int64_t l = w / B, i = w - l * B;
      if (i < nf) {
        const int64_t row = (int64_t)frontier[i] * L + l;
        const int32_t deg = rowptr[row + 1] - rowptr[row];
        c = (k == 0 || deg <= k) ? deg : k;
      }
    }
    counts[w] = c;
  }
}

__device__ __forceinline__ uint64_t key_of(int32_t j, uint32_t row, uint32_t hop, uint32_t draw, uint32_t k0, uint32_t k1) {
  const u32x4 r = philox4x32_10((uint32_t)j >> 2, row, hop, draw, k0, k1);
  const int e = j & 3;
  const uint32_t word = e == 0 ? r.x : e == 1 ? r.y : e == 2 ? r.z : r.w;
  return ((uint64_t)word << 32) | (uint32_t)j;
}

// the three smallest keys, ascending, among this lane's positions (lane, lane + 64, ... < deg) that are above `after` (every key
// when !bounded); all ones where the lane has fewer (no key is all ones: a position is below 2^31)
struct LaneKeys { uint64_t q0, q1, q2; };

__device__ __forceinline__ LaneKeys lane_smallest(int lane, int32_t deg, bool bounded, uint64_t after, uint32_t row, uint32_t hop,
                                                  uint32_t draw, uint32_t k0, uint32_t k1) {
  LaneKeys s = {~0ull, ~0ull, ~0ull};
  for (int32_t j = lane; j < deg; j += RELGNN_WAVE) {
    const uint64_t key = key_of(j, row, hop, draw, k0, k1);
    if (bounded && key <= after) continue;
    if (key < s.q0) { s.q2 = s.q1; s.q1 = s.q0; s.q0 = key; }
    else if (key < s.q1) { s.q2 = s.q1; s.q1 = key; }
    else if (key < s.q2) s.q2 = key;
  }
  return s;
}

__device__ __forceinline__ void emit(int64_t slot, int64_t edge_bound, int32_t source_row, int32_t L, int32_t target, int64_t V,
                                     int32_t mark, int32_t* __restrict__ stamp, int2* __restrict__ edges) {
  const int32_t src = source_row / L;
  if (slot < edge_bound) edges[slot] = make_int2(src, target);
  if ((uint32_t)src < (uint64_t)V && stamp[src] == 0) stamp[src] = mark;      // every writer of this hop writes `mark`
}

__global__ __launch_bounds__(256) void take_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                   int32_t L, const int32_t* __restrict__ frontier,
                                                   const int32_t* __restrict__ frontier_count, int64_t B, int32_t k, uint32_t hop,
                                                   uint32_t draw, uint32_t k0, uint32_t k1, const int32_t* __restrict__ offsets,
                                                   int64_t edge_bound, int32_t* __restrict__ stamp, int2* __restrict__ edges) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t nf = set_size(frontier_count, B), total = B * L;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  const int32_t mark = (int32_t)hop + 1;
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + (threadIdx.x / RELGNN_WAVE); w < total; w += waves) {
    const int64_t l = w / B, i = w - l * B;
    if (i >= nf) continue;                                   // (the same in every lane of the wave, like every branch below but one)
    const int32_t t = frontier[i];
    const int64_t row = (int64_t)t * L + l;
    const int32_t b = rowptr[row], deg = rowptr[row + 1] - b;
    const int64_t off = offsets[w];
    if (k == 0 || deg <= k) {
      for (int32_t j = lane; j < deg; j += RELGNN_WAVE) emit(off + j, edge_bound, col[b + j], L, t, V, mark, stamp, edges);
      continue;
    }
    LaneKeys s = lane_smallest(lane, deg, false, 0, (uint32_t)row, hop, draw, k0, k1);
    int known = 3;                                           // how many of s.q0, s.q1, s.q2 are still this lane's smallest untaken keys
    int32_t mine = 0x7fffffff;                               // lane r: the position taken in round r
    for (int r = 0; r < k; ++r) {
      uint64_t m = s.q0;
#pragma unroll
      for (int d = RELGNN_WAVE / 2; d >= 1; d >>= 1) {
        const uint64_t other = __shfl_xor(m, d);
        m = other < m ? other : m;
      }
      if (lane == r) mine = (int32_t)(uint32_t)m;
      if (s.q0 == m) {                                       // keys are distinct: one lane, which moves on to its next key
        s.q0 = s.q1; s.q1 = s.q2; s.q2 = ~0ull;
        if (--known == 0) {                                  // the third win of a lane since its last walk: walk again, above m
          s = lane_smallest(lane, deg, true, m, (uint32_t)row, hop, draw, k0, k1);
          known = 3;
        }
      }
    }
    int rank = 0;
    for (int q = 0; q < k; ++q) rank += __shfl(mine, q) < mine ? 1 : 0;
    if (lane < k) emit(off + rank, edge_bound, col[b + mine], L, t, V, mark, stamp, edges);
  }
}

__global__ __launch_bounds__(256) void scatter_kernel(const int32_t* __restrict__ stamp, const int32_t* __restrict__ pos, int64_t V,
                                                      StampFlag flag, int32_t* __restrict__ out, int64_t capacity,
                                                      int32_t* __restrict__ count) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t f = flag(stamp[v]), p = pos[v];
    if (f && p < capacity) out[p] = (int32_t)v;
    if (v == V - 1) {
      const int64_t n = (int64_t)p + f;
      *count = (int32_t)(n < capacity ? n : capacity);
    }
  }
}

// position of v in the ascending list nodes[0 .. n): at most 32 halvings; a node that is not there (never, for what the hops
// emitted) gives an index inside the list all the same
__device__ __forceinline__ int32_t local_id(const int32_t* __restrict__ nodes, int64_t n, int32_t v) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (nodes[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (int32_t)(lo < n ? lo : n - 1);
}

__global__ __launch_bounds__(256) void relabel_kernel(const int2* __restrict__ edges, int64_t count, const int32_t* __restrict__ nodes,
                                                      int64_t n, int2* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
    const int2 st = edges[e];
    out[e] = make_int2(local_id(nodes, n, st.x), local_id(nodes, n, st.y));
  }
}

__global__ __launch_bounds__(256) void degrees_kernel(const int32_t* __restrict__ counts, int64_t B, int64_t nf, int32_t L,
                                                      const int32_t* __restrict__ frontier, const int32_t* __restrict__ nodes, int64_t n,
                                                      float* __restrict__ degrees) {
  const int64_t total = nf * L;
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = w / nf, i = w - l * nf;
    degrees[l * n + local_id(nodes, n, frontier[i])] = (float)counts[l * B + i];
  }
}

// ---- hop-ordered numbering (NeighbourSampler.sample_by_hop) -------------------------------------------------------------------------
// nodes = [seeds | first reached in hop 1 | ... | first reached in hop H], every segment ascending; start[d] is where the nodes at
// distance d begin, start[levels] = n.  A node's distance is in its stamp until finish clears it (-1: a seed).
struct HopStarts { int64_t start[kMaxHops + 2]; };

// start[d] + the rank of v inside segment d: the bounded search of local_id over one segment; a node that is not there (never, for
// what the hops emitted) gives an index inside the list all the same
__device__ __forceinline__ int32_t hop_local_id(const int32_t* __restrict__ stamp, int64_t V, const int32_t* __restrict__ nodes,
                                                const HopStarts& hs, int32_t levels, int32_t v) {
  int32_t d = 0;
  if ((uint32_t)v < (uint64_t)V) d = stamp[v];
  d = d < 0 ? 0 : (d >= levels ? levels - 1 : d);
  const int64_t lo = hs.start[d], hi = hs.start[d + 1], n = hs.start[levels];
  const int64_t at = hi > lo ? lo + local_id(nodes + lo, hi - lo, v) : lo;
  return (int32_t)(at < n ? at : n - 1);
}

__global__ __launch_bounds__(256) void relabel_by_hop_kernel(const int2* __restrict__ edges, int64_t count,
                                                             const int32_t* __restrict__ stamp, int64_t V,
                                                             const int32_t* __restrict__ nodes, HopStarts hs, int32_t levels,
                                                             int2* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
    const int2 st = edges[e];
    out[e] = make_int2(hop_local_id(stamp, V, nodes, hs, levels, st.x), hop_local_id(stamp, V, nodes, hs, levels, st.y));
  }
}

// the frontier of a hop is the local range [base, base + nf): its degree columns are a strided copy of counts
__global__ __launch_bounds__(256) void degrees_by_hop_kernel(const int32_t* __restrict__ counts, int64_t B, int64_t nf, int32_t L,
                                                             int64_t base, int64_t n, float* __restrict__ degrees) {
  const int64_t total = nf * L;
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = w / nf, i = w - l * nf;
    if (base + i < n) degrees[l * n + base + i] = (float)counts[l * B + i];
  }
}

__global__ __launch_bounds__(256) void finish_kernel(const int32_t* __restrict__ nodes, int64_t n, int32_t* __restrict__ stamp, int64_t V,
                                                     float* __restrict__ seed_mask) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = nodes[i];
    float m = 0.f;
    if ((uint32_t)v < (uint64_t)V) {
      m = stamp[v] == kSeedStamp ? 1.f : 0.f;
      stamp[v] = 0;
    }
    seed_mask[i] = m;
  }
}

}  // namespace

extern "C" {

int relgnn_neighbour_sample_supported(const int32_t* fanouts, int32_t num_hops, int64_t num_nodes, int32_t num_edge_types) {
  if (!fanouts || num_hops < 1 || num_hops > kMaxHops || !graph_ok(num_nodes, num_edge_types)) return 0;
  for (int32_t h = 0; h < num_hops; ++h)
    if (fanouts[h] < 0 || fanouts[h] > kMaxFanout) return 0;
  return 1;
}

int64_t relgnn_neighbour_sample_max_fanout(void) { return kMaxFanout; }
int64_t relgnn_neighbour_sample_max_hops(void) { return kMaxHops; }

size_t relgnn_neighbour_sample_workspace_bytes(int64_t max_items) {
  if (max_items < 1) max_items = 1;
  // [positions of a compaction: max_items int32 | rocPRIM's scan storage, for a hop's counts or a compaction's flags]
  return align_up((size_t)max_items * 4, 256) + align_up(scan_temp_bytes<true>(max_items + 1), 256) + 256;
}

int relgnn_neighbour_sample_begin(const int32_t* seeds, int64_t num_seeds, int32_t* stamp, int64_t num_nodes, void* stream) {
  if (num_seeds < 0 || num_nodes <= 0) return RELGNN_EINVAL;
  if (num_seeds == 0) return RELGNN_OK;
  if (!seeds || !stamp) return RELGNN_EINVAL;
  begin_kernel<<<flat_grid(num_seeds, 256), 256, 0, as_stream(stream)>>>(seeds, num_seeds, stamp, num_nodes);
  return launch_status();
}

int relgnn_neighbour_sample_count(const int32_t* rowptr_t, int64_t num_nodes, int32_t num_edge_types, const int32_t* frontier,
                                  const int32_t* frontier_count, int64_t frontier_bound, int32_t fanout, int32_t* counts,
                                  int32_t* offsets, int32_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  if (frontier_bound <= 0 || frontier_bound > num_nodes) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types) || fanout < 0 || fanout > kMaxFanout) return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !frontier || !frontier_count || !counts || !offsets || !totals || !workspace) return RELGNN_EINVAL;
  const int64_t items = frontier_bound * num_edge_types + 1;
  if (workspace_bytes < relgnn_neighbour_sample_workspace_bytes(items)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  count_kernel<<<flat_grid(items, 256), 256, 0, st>>>(rowptr_t, num_edge_types, frontier, frontier_count, frontier_bound, fanout, counts);
  const size_t front = align_up((size_t)items * 4, 256);          // (the scan storage lies where a compaction's does)
  return scan_bucket_counts(counts, offsets, frontier_bound, num_edge_types, totals, static_cast<char*>(workspace) + front,
                            workspace_bytes - front, st);
}

int relgnn_neighbour_sample_take(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                 const int32_t* frontier, const int32_t* frontier_count, int64_t frontier_bound, int32_t fanout,
                                 int32_t hop, uint32_t draw, uint32_t seed, uint32_t replica, const int32_t* offsets,
                                 int64_t edge_bound, int32_t* stamp, int32_t* edges, void* stream) {
  if (frontier_bound <= 0 || frontier_bound > num_nodes || edge_bound < 0) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types) || fanout < 0 || fanout > kMaxFanout || hop < 0 || hop >= kMaxHops)
    return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !col_t || !frontier || !frontier_count || !offsets || !stamp || (edge_bound > 0 && !edges)) return RELGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(edges) & 7u) return RELGNN_EINVAL;
  const int64_t buckets = frontier_bound * num_edge_types;
  take_kernel<<<flat_grid(buckets * RELGNN_WAVE, 256), 256, 0, as_stream(stream)>>>(
      rowptr_t, col_t, num_nodes, num_edge_types, frontier, frontier_count, frontier_bound, fanout, (uint32_t)hop, draw, seed,
      0x80000000u | replica, offsets, edge_bound, stamp, reinterpret_cast<int2*>(edges));
  return launch_status();
}

int relgnn_neighbour_sample_compact(const int32_t* stamp, int64_t num_nodes, int32_t value, int32_t* out, int64_t out_capacity,
                                    int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  if (num_nodes <= 0 || out_capacity < 0 || value < 0) return RELGNN_EINVAL;
  if (num_nodes >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (!stamp || !count || !workspace || (out_capacity > 0 && !out)) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_neighbour_sample_workspace_bytes(num_nodes)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  int32_t* pos = static_cast<int32_t*>(workspace);
  const size_t front = align_up((size_t)num_nodes * 4, 256);
  size_t temp_bytes = workspace_bytes - front;
  const StampFlag flag{value};
  if (rocprim::exclusive_scan(static_cast<char*>(workspace) + front, temp_bytes, rocprim::make_transform_iterator(stamp, flag), pos,
                              (int32_t)0, (size_t)num_nodes, rocprim::plus<int32_t>(), st) != hipSuccess)
    return RELGNN_EHIP;
  scatter_kernel<<<flat_grid(num_nodes, 256), 256, 0, st>>>(stamp, pos, num_nodes, flag, out, out_capacity, count);
  return launch_status();
}

int relgnn_neighbour_sample_relabel(const int32_t* edges, int64_t first, int64_t count, const int32_t* nodes, int64_t n,
                                    int32_t* out, void* stream) {
  if (first < 0 || count < 0 || n < 0) return RELGNN_EINVAL;
  if (count == 0) return RELGNN_OK;
  if (!edges || !nodes || !out || n == 0) return RELGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(edges) | reinterpret_cast<uintptr_t>(out)) & 7u) return RELGNN_EINVAL;
  relabel_kernel<<<flat_grid(count, 256), 256, 0, as_stream(stream)>>>(reinterpret_cast<const int2*>(edges) + first, count, nodes, n,
                                                                       reinterpret_cast<int2*>(out));
  return launch_status();
}

int relgnn_neighbour_sample_degrees(const int32_t* counts, int64_t frontier_bound, int64_t frontier_count, int32_t num_edge_types,
                                    const int32_t* frontier, const int32_t* nodes, int64_t n, float* degrees, void* stream) {
  if (frontier_count < 0 || frontier_count > frontier_bound || num_edge_types <= 0 || n < 0) return RELGNN_EINVAL;
  if (frontier_count == 0) return RELGNN_OK;
  if (!counts || !frontier || !nodes || !degrees || n == 0) return RELGNN_EINVAL;
  degrees_kernel<<<flat_grid(frontier_count * num_edge_types, 256), 256, 0, as_stream(stream)>>>(
      counts, frontier_bound, frontier_count, num_edge_types, frontier, nodes, n, degrees);
  return launch_status();
}

int relgnn_neighbour_sample_relabel_by_hop(const int32_t* edges, int64_t first, int64_t count, const int32_t* stamp,
                                           int64_t num_nodes, const int32_t* nodes, const int64_t* hop_starts, int32_t num_levels,
                                           int32_t* out, void* stream) {
  if (first < 0 || count < 0 || num_nodes <= 0 || !hop_starts) return RELGNN_EINVAL;
  if (num_levels < 1 || num_levels > kMaxHops + 1) return RELGNN_EUNSUPPORTED;
  HopStarts hs = {};
  for (int32_t d = 0; d <= num_levels; ++d) {
    hs.start[d] = hop_starts[d];
    if (hs.start[d] < 0 || (d == 0 ? hs.start[d] != 0 : hs.start[d] < hs.start[d - 1])) return RELGNN_EINVAL;
  }
  if (hs.start[num_levels] >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (count == 0) return RELGNN_OK;
  if (!edges || !stamp || !nodes || !out || hs.start[num_levels] == 0) return RELGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(edges) | reinterpret_cast<uintptr_t>(out)) & 7u) return RELGNN_EINVAL;
  relabel_by_hop_kernel<<<flat_grid(count, 256), 256, 0, as_stream(stream)>>>(reinterpret_cast<const int2*>(edges) + first, count, stamp,
                                                                              num_nodes, nodes, hs, num_levels,
                                                                              reinterpret_cast<int2*>(out));
  return launch_status();
}

int relgnn_neighbour_sample_degrees_by_hop(const int32_t* counts, int64_t frontier_bound, int64_t frontier_count,
                                           int32_t num_edge_types, int64_t base, int64_t n, float* degrees, void* stream) {
  if (frontier_count < 0 || frontier_count > frontier_bound || num_edge_types <= 0 || base < 0 || n < 0) return RELGNN_EINVAL;
  if (base + frontier_count > n) return RELGNN_EINVAL;
  if (frontier_count == 0) return RELGNN_OK;
  if (!counts || !degrees) return RELGNN_EINVAL;
  degrees_by_hop_kernel<<<flat_grid(frontier_count * num_edge_types, 256), 256, 0, as_stream(stream)>>>(
      counts, frontier_bound, frontier_count, num_edge_types, base, n, degrees);
  return launch_status();
}

int relgnn_neighbour_sample_finish(const int32_t* nodes, int64_t n, int32_t* stamp, int64_t num_nodes, float* seed_mask,
                                   void* stream) {
  if (n < 0 || num_nodes <= 0) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!nodes || !stamp || !seed_mask) return RELGNN_EINVAL;
  finish_kernel<<<flat_grid(n, 256), 256, 0, as_stream(stream)>>>(nodes, n, stamp, num_nodes, seed_mask);
  return launch_status();
}

}  // extern "C"
