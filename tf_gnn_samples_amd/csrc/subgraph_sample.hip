// Subgraph sampling for single-graph node classification (include/relgnn_subgraph.h states the rules; tasks/subgraph_sampling.py
// drives the calls): random walks against the edges of the full graph's by-target bucketing, read in place, and the node-induced
// subgraph over the stamped node set.
//
// One LANE owns one walk: a step is two rowptr loads, one Philox call and one col load; the walk's nodes are stamped with plain
// stores of the one value every writer writes.  The stamp array and what its values mean are node_set.h's; the node list is the node
// set's compaction (relgnn_neighbour_sample_compact, a flag scan over the stamps, defined in neighbour_sample.hip).
// One WAVE owns one (subgraph node, edge type) bucket of the full graph, of any length: the lanes stride over it 64 entries at a
// pass (the loads of eight passes are issued together); an entry is kept when its source is stamped.  The count is the popcount of
// the pass's ballot; offsets and per-type totals are node_set.h's scan_bucket_counts, as for a hop of neighbour sampling.  The emit
// walks the bucket the same way: a kept entry's slot is the bucket's offset + the kept entries of the earlier passes + the popcount
// of the kept-mask below the lane, so the kept entries come out in the bucket's own order.  A source's local id is its stamp - 1
// (relgnn_subgraph_number wrote the positions into the stamps), the target's is the bucket's position in the node list.  Every loop
// is bounded by a bucket length or a launch argument.  No atomics anywhere.
//
// GraphSAINT normalisation (include/relgnn_subgraph_norm.h): the visit count walks the buckets as the count does and adds 1 to the
// position of every kept entry and to the node of every type-0 wave, plain load-add-store: a position belongs to one lane of one
// wave of a launch, and the launches of a stream are ordered.  The weighted emit is the emit with one more store per kept entry.
#include "node_set.h"
#include "philox.h"
#include "../../include/relgnn_subgraph.h"
#include "../../include/relgnn_subgraph_norm.h"

using namespace relgnn;

namespace {

constexpr int kMaxWalkLength = 64;
constexpr int32_t kWalkStamp = 1;
constexpr int kPasses = 8;                  // 64-entry passes of a bucket whose loads are in flight together

__global__ __launch_bounds__(256) void walk_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                   int32_t L, const int32_t* __restrict__ roots, int64_t R, int32_t h, uint32_t draw,
                                                   uint32_t k0, uint32_t k1, int32_t* __restrict__ stamp) {
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < R; w += (int64_t)gridDim.x * blockDim.x) {
    int32_t v = roots[w];
    if ((uint32_t)v >= (uint64_t)V) continue;                   // (never, for a validated root list)
    stamp[v] = kWalkStamp;
    for (int32_t s = 0; s < h; ++s) {
      const int32_t b = rowptr[(int64_t)v * L], deg = rowptr[(int64_t)(v + 1) * L] - b;
      if (deg <= 0) break;                                      // a dead end: every later step stays here too
      const uint32_t word = philox4x32_10((uint32_t)w, (uint32_t)s, draw, 0u, k0, k1).x;
      const int32_t next = col[(int64_t)b + __umulhi(word, (uint32_t)deg)] / L;
      if ((uint32_t)next >= (uint64_t)V) break;                 // (never, for a checked graph)
      v = next;
      stamp[v] = kWalkStamp;
    }
  }
}

__global__ __launch_bounds__(256) void number_kernel(const int32_t* __restrict__ nodes, const int32_t* __restrict__ count, int64_t B,
                                                     int32_t* __restrict__ stamp, int64_t V) {
  const int64_t n = set_size(count, B);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = nodes[i];
    if ((uint32_t)v < (uint64_t)V) stamp[v] = (int32_t)i + 1;
  }
}

// is the source of a bucket entry in the set?  (its stamp, 0 where it is not)
__device__ __forceinline__ int32_t source_stamp(int32_t source_row, int32_t L, int64_t V, const int32_t* __restrict__ stamp) {
  const int32_t src = source_row / L;
  return source_row >= 0 && (uint32_t)src < (uint64_t)V ? stamp[src] : 0;
}

// s[u] = the stamp of the source of bucket entry j + u * 64 (0 beyond the bucket's deg entries), u in [0, kPasses): the loads of
// kPasses 64-entry passes are issued together, first the entries, then their stamps; a hub bucket is one wave's serial walk, and
// its time is the number of dependent round trips to memory
__device__ __forceinline__ void load_stamps(const int32_t* __restrict__ bucket, int32_t j, int32_t deg, int32_t L, int64_t V,
                                            const int32_t* __restrict__ stamp, int32_t (&s)[kPasses]) {
  int32_t entry[kPasses];
#pragma unroll
  for (int u = 0; u < kPasses; ++u) {
    const int64_t at = (int64_t)j + u * RELGNN_WAVE;
    entry[u] = at < deg ? bucket[at] : -1;
  }
#pragma unroll
  for (int u = 0; u < kPasses; ++u) s[u] = source_stamp(entry[u], L, V, stamp);
}

// counts[l * B + i] = kept entries of bucket (nodes[i], l); 0 beyond the set and in the closing entry
__global__ __launch_bounds__(256) void induced_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            int64_t V, int32_t L, const int32_t* __restrict__ nodes,
                                                            const int32_t* __restrict__ count, int64_t B,
                                                            const int32_t* __restrict__ stamp, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t n = set_size(count, B), total = B * L;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + (threadIdx.x / RELGNN_WAVE); w <= total; w += waves) {
    int32_t kept = 0;                                           // (the same in every lane of the wave, like every branch but one)
    if (w < total) {
      const int64_t l = w / B, i = w - l * B;
      if (i < n) {
        const int32_t t = nodes[i];
        if ((uint32_t)t < (uint64_t)V) {
          const int64_t row = (int64_t)t * L + l;
          const int32_t b = rowptr[row], deg = rowptr[row + 1] - b;
          for (int32_t first = 0; first < deg; first += kPasses * RELGNN_WAVE) {
            int32_t s[kPasses];
            load_stamps(col + b, first + lane, deg, L, V, stamp, s);
#pragma unroll
            for (int u = 0; u < kPasses; ++u) kept += __popcll(__ballot(s[u] != 0));
          }
        }
      }
    }
    if (lane == 0) counts[w] = kept;
  }
}

// one pre-sampled subgraph: edge_visits[b + j] += 1 for every kept entry j of bucket (nodes[i], l), node_visits[nodes[i]] += 1 from the
// wave of type 0.  One writer per address (a node is in the list once; a position belongs to one lane in one pass): no atomics.
__global__ __launch_bounds__(256) void visit_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                          int32_t L, int64_t M, const int32_t* __restrict__ nodes,
                                                          const int32_t* __restrict__ count, int64_t B,
                                                          const int32_t* __restrict__ stamp, int32_t* __restrict__ node_visits,
                                                          int32_t* __restrict__ edge_visits) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t n = set_size(count, B), total = n * L;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + (threadIdx.x / RELGNN_WAVE); w < total; w += waves) {
    const int64_t l = w / n, i = w - l * n;
    const int32_t t = nodes[i];
    if ((uint32_t)t >= (uint64_t)V) continue;
    if (l == 0 && lane == 0) node_visits[t] += 1;
    const int64_t row = (int64_t)t * L + l;
    const int32_t b = rowptr[row], deg = rowptr[row + 1] - b;
    for (int32_t first = 0; first < deg; first += kPasses * RELGNN_WAVE) {
      int32_t s[kPasses];
      load_stamps(col + b, first + lane, deg, L, V, stamp, s);
#pragma unroll
      for (int u = 0; u < kPasses; ++u) {
        const int64_t p = (int64_t)b + first + lane + u * RELGNN_WAVE;
        if (s[u] != 0 && p < M) edge_visits[p] += 1;
      }
    }
  }
}

// what a weighted emit reads and writes on top (include/relgnn_subgraph_norm.h); kWeighted == false: not touched
struct EmitWeights {
  const int32_t* node_visits;
  const int32_t* edge_visits;
  float* edge_weights;
  int64_t M;
  float cap;
};

template <bool kWeighted>
__global__ __launch_bounds__(256) void induced_emit_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t V,
                                                           int32_t L, const int32_t* __restrict__ nodes, int64_t n, int64_t B,
                                                           const int32_t* __restrict__ stamp, const int32_t* __restrict__ offsets,
                                                           int64_t edge_bound, int2* __restrict__ edges, float* __restrict__ degrees,
                                                           EmitWeights ew) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t total = n * L;
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  for (int64_t w = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + (threadIdx.x / RELGNN_WAVE); w < total; w += waves) {
    const int64_t l = w / n, i = w - l * n;
    const int32_t t = nodes[i];
    int32_t kept = 0;
    if ((uint32_t)t < (uint64_t)V) {
      const int64_t row = (int64_t)t * L + l;
      const int32_t b = rowptr[row], deg = rowptr[row + 1] - b;
      const int64_t off = offsets[l * B + i];
      float visits = 1.f, scale = 0.f;                          // (kWeighted) max(C_t, 1) and the full graph's 1 / (deg + 1e-7)
      if constexpr (kWeighted) {
        const int32_t c = ew.node_visits[t];
        visits = (float)(c > 1 ? c : 1);
        scale = 1.0f / ((float)deg + 1e-7f);
      }
      for (int32_t first = 0; first < deg; first += kPasses * RELGNN_WAVE) {
        int32_t s[kPasses];
        load_stamps(col + b, first + lane, deg, L, V, stamp, s);
#pragma unroll
        for (int u = 0; u < kPasses; ++u) {                     // the passes in the bucket's order
          const unsigned long long mask = __ballot(s[u] != 0);
          const int64_t slot = off + kept + __popcll(mask & below);
          if (s[u] != 0 && slot < edge_bound) {
            const int64_t local = (int64_t)s[u] - 1;            // number_kernel's position, inside the list all the same
            edges[slot] = make_int2((int32_t)(local < 0 ? 0 : (local < n ? local : n - 1)), (int32_t)i);
            if constexpr (kWeighted) {
              const int64_t p = (int64_t)b + first + lane + u * RELGNN_WAVE;
              const int32_t c = p < ew.M ? ew.edge_visits[p] : 1;
              const float a = fminf(visits / (float)(c > 1 ? c : 1), ew.cap);
              ew.edge_weights[slot] = a * scale;
            }
          }
          kept += __popcll(mask);
        }
      }
    }
    if (lane == 0) degrees[l * n + i] = (float)kept;
  }
}

__global__ __launch_bounds__(256) void clear_kernel(const int32_t* __restrict__ nodes, int64_t n, int32_t* __restrict__ stamp, int64_t V) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = nodes[i];
    if ((uint32_t)v < (uint64_t)V) stamp[v] = 0;
  }
}

}  // namespace

extern "C" {

int relgnn_subgraph_supported(int64_t num_walks, int32_t walk_length, int64_t num_nodes, int32_t num_edge_types) {
  return num_walks >= 1 && walk_length >= 0 && walk_length <= kMaxWalkLength && graph_ok(num_nodes, num_edge_types) ? 1 : 0;
}

int64_t relgnn_subgraph_max_walk_length(void) { return kMaxWalkLength; }

size_t relgnn_subgraph_workspace_bytes(int64_t max_items) {
  if (max_items < 1) max_items = 1;
  return align_up(scan_temp_bytes<false>(max_items), 256) + 256;      // the plain scan alone: nothing is compacted in here
}

int relgnn_subgraph_walk(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                         const int32_t* roots, int64_t num_walks, int32_t walk_length, uint32_t draw, uint32_t seed,
                         uint32_t replica, int32_t* stamp, void* stream) {
  if (num_walks < 1 || num_nodes <= 0) return RELGNN_EINVAL;
  if (!relgnn_subgraph_supported(num_walks, walk_length, num_nodes, num_edge_types)) return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !roots || !stamp || (walk_length > 0 && !col_t)) return RELGNN_EINVAL;
  walk_kernel<<<flat_grid(num_walks, 256), 256, 0, as_stream(stream)>>>(rowptr_t, col_t, num_nodes, num_edge_types, roots, num_walks,
                                                                        walk_length, draw, seed, replica, stamp);
  return launch_status();
}

int relgnn_subgraph_number(const int32_t* nodes, const int32_t* node_count, int64_t node_bound, int32_t* stamp, int64_t num_nodes,
                           void* stream) {
  if (node_bound <= 0 || num_nodes <= 0 || node_bound > num_nodes) return RELGNN_EINVAL;
  if (num_nodes >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (!nodes || !node_count || !stamp) return RELGNN_EINVAL;
  number_kernel<<<flat_grid(node_bound, 256), 256, 0, as_stream(stream)>>>(nodes, node_count, node_bound, stamp, num_nodes);
  return launch_status();
}

int relgnn_subgraph_induced_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                  const int32_t* nodes, const int32_t* node_count, int64_t node_bound, const int32_t* stamp,
                                  int32_t* counts, int32_t* offsets, int32_t* totals, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (node_bound <= 0 || node_bound > num_nodes) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types)) return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !col_t || !nodes || !node_count || !stamp || !counts || !offsets || !totals || !workspace) return RELGNN_EINVAL;
  const int64_t items = node_bound * num_edge_types + 1;
  if (workspace_bytes < relgnn_subgraph_workspace_bytes(items)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  induced_count_kernel<<<flat_grid(items * RELGNN_WAVE, 256), 256, 0, st>>>(rowptr_t, col_t, num_nodes, num_edge_types, nodes, node_count,
                                                                            node_bound, stamp, counts);
  return scan_bucket_counts(counts, offsets, node_bound, num_edge_types, totals, workspace, workspace_bytes, st);
}

int relgnn_subgraph_induced_emit(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                 const int32_t* nodes, int64_t n, int64_t node_bound, const int32_t* stamp, const int32_t* offsets,
                                 int64_t edge_bound, int32_t* edges, float* degrees, void* stream) {
  if (n < 0 || node_bound <= 0 || n > node_bound || node_bound > num_nodes || edge_bound < 0) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types)) return RELGNN_EUNSUPPORTED;
  if (n == 0) return RELGNN_OK;
  if (!rowptr_t || !col_t || !nodes || !stamp || !offsets || !degrees || (edge_bound > 0 && !edges)) return RELGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(edges) & 7u) return RELGNN_EINVAL;
  induced_emit_kernel<false><<<flat_grid(n * num_edge_types * RELGNN_WAVE, 256), 256, 0, as_stream(stream)>>>(
      rowptr_t, col_t, num_nodes, num_edge_types, nodes, n, node_bound, stamp, offsets, edge_bound, reinterpret_cast<int2*>(edges),
      degrees, EmitWeights{nullptr, nullptr, nullptr, 0, 0.f});
  return launch_status();
}

int relgnn_subgraph_visit_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                int64_t num_messages, const int32_t* nodes, const int32_t* node_count, int64_t node_bound,
                                const int32_t* stamp, int32_t* node_visits, int32_t* edge_visits, void* stream) {
  if (node_bound <= 0 || node_bound > num_nodes || num_messages < 0) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types) || num_messages >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (!rowptr_t || !nodes || !node_count || !stamp || !node_visits || (num_messages > 0 && (!col_t || !edge_visits))) return RELGNN_EINVAL;
  visit_count_kernel<<<flat_grid(node_bound * num_edge_types * RELGNN_WAVE, 256), 256, 0, as_stream(stream)>>>(
      rowptr_t, col_t, num_nodes, num_edge_types, num_messages, nodes, node_count, node_bound, stamp, node_visits, edge_visits);
  return launch_status();
}

int relgnn_subgraph_induced_emit_weighted(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                                          int64_t num_messages, const int32_t* nodes, int64_t n, int64_t node_bound,
                                          const int32_t* stamp, const int32_t* offsets, const int32_t* node_visits,
                                          const int32_t* edge_visits, float max_edge_weight, int64_t edge_bound, int32_t* edges,
                                          float* degrees, float* edge_weights, void* stream) {
  if (n < 0 || node_bound <= 0 || n > node_bound || node_bound > num_nodes || edge_bound < 0 || num_messages < 0) return RELGNN_EINVAL;
  if (!(max_edge_weight > 0.f)) return RELGNN_EINVAL;
  if (!graph_ok(num_nodes, num_edge_types) || num_messages >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (n == 0) return RELGNN_OK;
  if (!rowptr_t || !col_t || !nodes || !stamp || !offsets || !degrees || !node_visits || (num_messages > 0 && !edge_visits) ||
      (edge_bound > 0 && (!edges || !edge_weights)))
    return RELGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(edges) & 7u) return RELGNN_EINVAL;
  induced_emit_kernel<true><<<flat_grid(n * num_edge_types * RELGNN_WAVE, 256), 256, 0, as_stream(stream)>>>(
      rowptr_t, col_t, num_nodes, num_edge_types, nodes, n, node_bound, stamp, offsets, edge_bound, reinterpret_cast<int2*>(edges),
      degrees, EmitWeights{node_visits, edge_visits, edge_weights, num_messages, max_edge_weight});
  return launch_status();
}

int relgnn_subgraph_clear(const int32_t* nodes, int64_t n, int32_t* stamp, int64_t num_nodes, void* stream) {
  if (n < 0 || num_nodes <= 0) return RELGNN_EINVAL;
  if (n == 0) return RELGNN_OK;
  if (!nodes || !stamp) return RELGNN_EINVAL;
  clear_kernel<<<flat_grid(n, 256), 256, 0, as_stream(stream)>>>(nodes, n, stamp, num_nodes);
  return launch_status();
}

}  // extern "C"
