// The block of a window of target rows of one graph (window_block.h states the rule; tasks/layerwise.py sizes the outputs from the one
// read-back and builds the LevelGraph): layer-wise full-graph evaluation computes a layer for the targets [first, last) from a stored
// table of the layer below, and the block is what that takes.  gfx950 only.
//
// The by-target bucketing is target-major: the entries of the targets [first, last) are one contiguous slice of col_t.  Launches per
// window, whatever a bucket's length:
//   count_kernel   flat over the T * L + 1 rows of the window: the bucket lengths, laid type-major as the sampler's counts are; node_set.h's
//                  scan_bucket_counts turns them into offsets and per-type totals.
//   stamp_kernel   flat over the slice, tiles of 1024 entries, one entry per lane: a source outside the window is stamped 1 (a plain
//                  store of the one value every writer writes).  The caller lists the stamps ascending with the node set's compaction.
//   emit_kernel    flat over the slice again: an entry finds its row by a binary search in rowptr_t[first * L .. last * L], its slot from
//                  the scanned counts and its source's local id by a binary search in the ascending list of outside sources.
//   finish_kernel  flat over max(n, L * n): nodes, the degree table, and the stamps of the listed sources back to zero.
// No atomics, no spin-wait, no hand-over between workgroups; no loop is bounded by a bucket's length.  Every store is checked against
// its buffer's length and every load against its array's: the sizes come from the host, and a wrong one must not become a fault.
#include "node_set.h"
#include "window_block.h"

using namespace relgnn;

namespace {

constexpr int kTile = 1024;                       // entries per workgroup of the two flat passes
constexpr int32_t kOutsideStamp = 1;

struct Window {
  int64_t V, M, first, T, base, E;                // nodes, messages, the first target, the targets, the slice's start and length
  int32_t L;
};

static inline unsigned tiles_of(int64_t E) { return (unsigned)((E + kTile - 1) / kTile); }

__global__ __launch_bounds__(256) void count_kernel(const int32_t* __restrict__ rowptr, Window w, int32_t* __restrict__ counts) {
  const int64_t total = w.T * w.L;
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x <= total; x += (int64_t)gridDim.x * blockDim.x) {
    int32_t c = 0;
    if (x < total) {
      const int64_t l = x / w.T, i = x - l * w.T;
      const int64_t row = (w.first + i) * w.L + l;                  // (< V * L: first + T <= V, checked on the host)
      c = rowptr[row + 1] - rowptr[row];
    }
    counts[x] = c < 0 ? 0 : c;
  }
}

__global__ __launch_bounds__(kTile) void stamp_kernel(const int32_t* __restrict__ col, Window w, int32_t* __restrict__ stamp) {
  const int64_t e = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (e >= w.E) return;
  const int64_t src = (int64_t)((uint32_t)col[w.base + e] / (uint32_t)w.L);   // (base + E <= M, checked on the host)
  if (src < w.V && (src < w.first || src >= w.first + w.T)) stamp[src] = kOutsideStamp;
}

// the row of by-target position p among rows[0 .. R]: the one r with rows[r] <= p < rows[r + 1] (empty rows share a start: the search
// passes over them); at most 32 halvings, and an index inside [0, R) whatever p and the row pointers are
__device__ __forceinline__ int64_t row_of(const int32_t* __restrict__ rows, int64_t R, int64_t p) {
  int64_t lo = 0, hi = R - 1;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rows[mid + 1] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the rank of v in the ascending list outside[0 .. n): at most 32 halvings; a node that is not there (never, for a list compacted
// from this window's stamps) gives an index inside the list all the same
__device__ __forceinline__ int64_t rank_in(const int32_t* __restrict__ outside, int64_t n, int32_t v) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (outside[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n ? lo : (n > 0 ? n - 1 : 0);
}

__global__ __launch_bounds__(kTile) void emit_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, Window w,
                                                     const int32_t* __restrict__ offsets, const int32_t* __restrict__ outside,
                                                     int64_t num_outside, int2* __restrict__ edges, int64_t edges_len) {
  const int64_t e = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (e >= w.E) return;
  const int64_t p = w.base + e;
  const int32_t* rows = rowptr + w.first * w.L;
  const int64_t r = row_of(rows, w.T * w.L, p);
  const int64_t i = r / w.L, l = r - i * w.L;
  const int64_t slot = (int64_t)offsets[l * w.T + i] + (p - rows[r]);
  const int64_t src = (int64_t)((uint32_t)col[p] / (uint32_t)w.L);
  int64_t local = src - w.first;
  if (local < 0 || local >= w.T) local = w.T + rank_in(outside, num_outside, (int32_t)src);
  if ((uint64_t)slot < (uint64_t)edges_len) edges[slot] = make_int2((int32_t)local, (int32_t)i);
}

__global__ __launch_bounds__(256) void finish_kernel(Window w, const int32_t* __restrict__ counts, const int32_t* __restrict__ outside,
                                                     int64_t num_outside, int32_t* __restrict__ stamp, int32_t* __restrict__ nodes,
                                                     int64_t nodes_len, float* __restrict__ degrees, int64_t degrees_len) {
  const int64_t n = w.T + num_outside, cells = n * w.L;
  for (int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; x < cells; x += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = x / n, i = x - l * n;
    if (x < degrees_len) degrees[x] = i < w.T ? (float)counts[l * w.T + i] : 0.f;
    if (l == 0) {
      int32_t id = (int32_t)(w.first + i);
      if (i >= w.T) {
        id = outside[i - w.T];
        if ((uint32_t)id < (uint64_t)w.V) stamp[id] = 0;
      }
      if (i < nodes_len) nodes[i] = id;
    }
  }
}

int window_status(const Window& w, int64_t last) {
  if (!graph_ok(w.V, w.L) || w.M >= ((int64_t)1 << 31)) return RELGNN_EUNSUPPORTED;
  if (w.first < 0 || w.first >= last || last > w.V || w.M < 0) return RELGNN_EINVAL;
  if (w.base < 0 || w.E < 0 || w.base > w.M || w.E > w.M - w.base) return RELGNN_EINVAL;
  return RELGNN_OK;
}

}  // namespace

extern "C" {

int relgnn_window_block_supported(int64_t num_nodes, int32_t num_edge_types) { return graph_ok(num_nodes, num_edge_types) ? 1 : 0; }

int64_t relgnn_window_block_tile(void) { return kTile; }

size_t relgnn_window_block_workspace_bytes(int64_t num_targets, int32_t num_edge_types) {
  if (num_targets < 1 || num_edge_types < 1) return 0;
  return align_up(scan_temp_bytes<false>(num_targets * num_edge_types + 1), 256) + 256;
}

int relgnn_window_block_count(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                              int64_t num_messages, int64_t first, int64_t last, int64_t entry_base, int64_t num_entries,
                              int32_t* stamp, int32_t* counts, int32_t* offsets, int32_t* totals, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const Window w = {num_nodes, num_messages, first, last - first, entry_base, num_entries, num_edge_types};
  const int status = window_status(w, last);
  if (status != RELGNN_OK) return status;
  if (!rowptr_t || !counts || !offsets || !totals || !workspace || (num_entries > 0 && (!col_t || !stamp))) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_window_block_workspace_bytes(w.T, w.L)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  count_kernel<<<flat_grid(w.T * w.L + 1, 256), 256, 0, st>>>(rowptr_t, w, counts);
  const int scanned = scan_bucket_counts(counts, offsets, w.T, w.L, totals, workspace, workspace_bytes, st);
  if (scanned != RELGNN_OK || num_entries == 0) return scanned;
  stamp_kernel<<<tiles_of(num_entries), kTile, 0, st>>>(col_t, w, stamp);
  return launch_status();
}

int relgnn_window_block_emit(const int32_t* rowptr_t, const int32_t* col_t, int64_t num_nodes, int32_t num_edge_types,
                             int64_t num_messages, int64_t first, int64_t last, int64_t entry_base, int64_t num_entries,
                             const int32_t* counts, const int32_t* offsets, const int32_t* outside, int64_t num_outside,
                             int32_t* stamp, int32_t* nodes, int64_t nodes_len, int32_t* edges, int64_t edges_len, float* degrees,
                             int64_t degrees_len, void* stream) {
  const Window w = {num_nodes, num_messages, first, last - first, entry_base, num_entries, num_edge_types};
  const int status = window_status(w, last);
  if (status != RELGNN_OK) return status;
  if (num_outside < 0 || num_outside > num_nodes - w.T || nodes_len < 0 || edges_len < 0 || degrees_len < 0) return RELGNN_EINVAL;
  if (!rowptr_t || !counts || !offsets || (nodes_len > 0 && !nodes) || (degrees_len > 0 && !degrees)) return RELGNN_EINVAL;
  if (num_outside > 0 && (!outside || !stamp)) return RELGNN_EINVAL;
  if (num_entries > 0 && (!col_t || (edges_len > 0 && !edges))) return RELGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(edges) & 7u) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  if (num_entries > 0)
    emit_kernel<<<tiles_of(num_entries), kTile, 0, st>>>(rowptr_t, col_t, w, offsets, outside, num_outside,
                                                         reinterpret_cast<int2*>(edges), edges_len);
  finish_kernel<<<flat_grid((w.T + num_outside) * w.L, 256), 256, 0, st>>>(w, counts, outside, num_outside, stamp, nodes, nodes_len,
                                                                          degrees, degrees_len);
  return launch_status();
}

}  // extern "C"
