// The level bucketings of a hop-ordered sampled batch, derived from the union graph's (level_plan.h states the rule;
// tasks/neighbour_sampling.py sizes the outputs from the hop sizes the sampler read back and builds the records).  gfx950 only.
//
// Five launches per batch, whatever the number of levels:
//   flag_kernel      flat over the M by-source entries, tiles of 1024 (16 waves): per wave and level the ballot mask of
//                    tgt_s[q] < T_d and, through LDS, the exclusive count of the waves in front of it in the tile; the tile's totals.
//   scan_kernel      ONE workgroup turns the tile totals into exclusive offsets, level by level (a thread sums a run of tiles, the
//                    1024 run sums are scanned in LDS, the thread writes its run's offsets).
//   compact_kernel   flat over the entries again: a kept entry goes to tile offset + wave offset + popcount(mask below its lane).
//   rowptr_kernel    flat over the rows: rowptr_t' is a copy and a fill, rowptr_s'[r] is the rank of entry rowptr_s[r], read from the
//                    same masks and offsets (two loads and a popcount per level).
//   by_target_kernel flat over the by-target positions: perm_t' and inv_perm_t' re-based by the per-type difference of list offsets.
// No atomics, no spin-wait, no hand-over between workgroups; no loop is bounded by a bucket's length.  Every store into `out` is
// checked against its length: the records come from the host, and a wrong one must not become a fault.
#include "common.h"
#include "level_plan.h"

using namespace relgnn;

namespace {

constexpr int kMaxLevels = 7;
constexpr int kTile = 1024;                       // entries per workgroup of the two flat passes
constexpr int kWaves = kTile / RELGNN_WAVE;       // 16
constexpr int kFixed = 11;                        // T, S, P and eight offsets in front of delta[L] and off'[L + 1]

enum Field { kT = 0, kS, kP, kRowptrT, kPermT, kInvPermT, kRowptrS, kTgtS, kFrowS, kPosS, kPermS };

struct Workspace {
  unsigned long long* mask;                       // [tiles * 16 * levels]: bit j of (chunk, level) = entry chunk * 64 + j is kept
  int32_t* wave_offset;                           // [tiles * 16 * levels]: kept entries of the tile in front of the chunk
  int32_t* tile_offset;                           // [tiles * levels]: the tile's total, then (scan_kernel) the kept entries in front of it
};

__host__ __device__ inline int64_t desc_stride(int32_t L) { return kFixed + 2 * (int64_t)L + 1; }

static inline int64_t tiles_of(int64_t M) { return (M + kTile - 1) / kTile; }

static Workspace carve(void* ws, int64_t M, int32_t D) {
  const size_t chunks = (size_t)tiles_of(M) * kWaves * D;
  char* p = static_cast<char*>(ws);
  Workspace w;
  w.mask = reinterpret_cast<unsigned long long*>(p);
  p += align_up(chunks * sizeof(unsigned long long), 256);
  w.wave_offset = reinterpret_cast<int32_t*>(p);
  p += align_up(chunks * sizeof(int32_t), 256);
  w.tile_offset = reinterpret_cast<int32_t*>(p);
  return w;
}

__device__ __forceinline__ void store_checked(int32_t* __restrict__ out, int64_t out_len, int64_t at, int32_t value) {
  if ((uint64_t)at < (uint64_t)out_len) out[at] = value;
}

// the kept entries of level d in front of by-source entry x (x < M)
__device__ __forceinline__ int32_t rank_of(const Workspace& w, int32_t D, int32_t d, int64_t x) {
  const int64_t chunk = x / RELGNN_WAVE, tile = x / kTile;
  const unsigned long long below = (1ull << (x % RELGNN_WAVE)) - 1ull;
  return w.tile_offset[tile * D + d] + w.wave_offset[chunk * D + d] + __popcll(w.mask[chunk * D + d] & below);
}

__global__ __launch_bounds__(kTile) void flag_kernel(const int32_t* __restrict__ tgt_s, int64_t M, const int64_t* __restrict__ desc,
                                                     int64_t stride, int32_t D, Workspace w) {
  __shared__ int32_t counts[kWaves][kMaxLevels];
  const int64_t q = (int64_t)blockIdx.x * kTile + threadIdx.x;
  const int wave = threadIdx.x / RELGNN_WAVE, lane = threadIdx.x % RELGNN_WAVE;
  const int64_t chunk = (int64_t)blockIdx.x * kWaves + wave;
  const int32_t target = q < M ? tgt_s[q] : 0x7fffffff;
  for (int d = 0; d < D; ++d) {
    const unsigned long long mask = __ballot(q < M && (int64_t)target < desc[d * stride + kT]);
    if (lane == 0) {
      w.mask[chunk * D + d] = mask;
      counts[wave][d] = __popcll(mask);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < D) {
    const int d = threadIdx.x;
    int32_t running = 0;
    for (int v = 0; v < kWaves; ++v) {
      w.wave_offset[((int64_t)blockIdx.x * kWaves + v) * D + d] = running;
      running += counts[v][d];
    }
    w.tile_offset[(int64_t)blockIdx.x * D + d] = running;
  }
}

__global__ __launch_bounds__(kTile) void scan_kernel(int64_t tiles, int32_t D, Workspace w) {
  __shared__ int32_t sums[kTile];
  const int t = threadIdx.x;
  const int64_t per = (tiles + kTile - 1) / kTile;
  const int64_t first = (int64_t)t * per < tiles ? (int64_t)t * per : tiles, last = first + per < tiles ? first + per : tiles;
  for (int d = 0; d < D; ++d) {
    int32_t mine = 0;
    for (int64_t b = first; b < last; ++b) mine += w.tile_offset[b * D + d];
    sums[t] = mine;
    __syncthreads();
    for (int step = 1; step < kTile; step <<= 1) {            // inclusive scan of the 1024 run sums
      const int32_t other = t >= step ? sums[t - step] : 0;
      __syncthreads();
      sums[t] += other;
      __syncthreads();
    }
    int32_t running = sums[t] - mine;
    for (int64_t b = first; b < last; ++b) {
      const int32_t total = w.tile_offset[b * D + d];
      w.tile_offset[b * D + d] = running;
      running += total;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kTile) void compact_kernel(const int32_t* __restrict__ tgt_s, const int32_t* __restrict__ frow_s,
                                                        const int32_t* __restrict__ pos_t_of_s, const int32_t* __restrict__ perm_s,
                                                        int64_t M, int32_t L, const int64_t* __restrict__ desc, int64_t stride, int32_t D,
                                                        Workspace w, int32_t* __restrict__ out, int64_t out_len) {
  const int64_t q = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (q >= M) return;
  const int32_t target = tgt_s[q], frow = frow_s[q], pos = pos_t_of_s[q], message = perm_s[q];
  const int32_t type = (uint32_t)frow % (uint32_t)L;
  for (int d = 0; d < D; ++d) {
    const int64_t* rec = desc + d * stride;
    if ((int64_t)target >= rec[kT]) continue;
    const int64_t at = rank_of(w, D, d, q);
    if (at < 0 || at >= rec[kP]) continue;                    // (never, for records that agree with the graph)
    store_checked(out, out_len, rec[kTgtS] + at, target);
    store_checked(out, out_len, rec[kFrowS] + at, frow);
    store_checked(out, out_len, rec[kPosS] + at, pos);
    store_checked(out, out_len, rec[kPermS] + at, (int32_t)(message - rec[kFixed + type]));
  }
}

__global__ void rowptr_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ rowptr_s, int64_t rows_in, int64_t M,
                              int32_t L, const int64_t* __restrict__ desc, int64_t stride, int32_t D, int64_t max_rows, Workspace w,
                              int32_t* __restrict__ out, int64_t out_len) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < max_rows; r += (int64_t)gridDim.x * blockDim.x) {
    if (r >= rows_in) continue;                               // (max_rows <= V * L + 1, checked on the host)
    const int32_t by_target = rowptr_t[r];
    const int64_t by_source = rowptr_s[r];
    for (int d = 0; d < D; ++d) {
      const int64_t* rec = desc + d * stride;
      if (r > rec[kS] * L) continue;
      const int32_t total = (int32_t)rec[kP];
      store_checked(out, out_len, rec[kRowptrT] + r, r <= rec[kT] * L ? by_target : total);
      const int32_t kept = (by_source < 0 || by_source >= M) ? total : rank_of(w, D, d, by_source);
      store_checked(out, out_len, rec[kRowptrS] + r, kept);
    }
  }
}

__global__ void by_target_kernel(const int32_t* __restrict__ col_t, const int32_t* __restrict__ perm_t,
                                 const int32_t* __restrict__ inv_perm_t, int64_t M, int32_t L, const int64_t* __restrict__ desc,
                                 int64_t stride, int32_t D, int64_t max_messages, int32_t* __restrict__ out, int64_t out_len) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < max_messages; p += (int64_t)gridDim.x * blockDim.x) {
    if (p >= M) continue;                                     // (max_messages <= M, checked on the host)
    const int32_t type = (uint32_t)col_t[p] % (uint32_t)L;
    const int32_t message = perm_t[p];
    for (int d = 0; d < D; ++d) {
      const int64_t* rec = desc + d * stride;
      if (p >= rec[kP]) continue;
      store_checked(out, out_len, rec[kPermT] + p, (int32_t)(message - rec[kFixed + type]));
      // the type of the level's message p: the last l with off'[l] <= p (empty types share a start: the search passes over them)
      const int64_t* offsets = rec + kFixed + L;
      int lo = 0, hi = L - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= p) lo = mid; else hi = mid - 1;
      }
      const int64_t in_union = p + rec[kFixed + lo];
      if (in_union >= 0 && in_union < M) store_checked(out, out_len, rec[kInvPermT] + p, inv_perm_t[in_union]);
    }
  }
}

}  // namespace

extern "C" {

int32_t relgnn_level_plan_max_levels(void) { return kMaxLevels; }

int64_t relgnn_level_plan_desc_stride(int32_t num_edge_types) { return num_edge_types < 1 ? 0 : desc_stride(num_edge_types); }

int64_t relgnn_level_plan_tile(void) { return kTile; }

size_t relgnn_level_plan_workspace_bytes(int64_t num_messages, int32_t num_levels) {
  if (num_messages <= 0 || num_levels <= 0 || num_levels > kMaxLevels) return 0;
  const size_t tiles = (size_t)tiles_of(num_messages), chunks = tiles * kWaves * num_levels;
  return align_up(chunks * sizeof(unsigned long long), 256) + align_up(chunks * sizeof(int32_t), 256) +
         align_up(tiles * num_levels * sizeof(int32_t), 256);
}

int relgnn_level_plan(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, const int32_t* inv_perm_t,
                      const int32_t* rowptr_s, const int32_t* tgt_s, const int32_t* frow_s, const int32_t* pos_t_of_s,
                      const int32_t* perm_s, int64_t num_nodes, int32_t num_edge_types, int64_t num_messages, const int64_t* desc,
                      int32_t num_levels, int64_t max_rows, int64_t max_messages, int32_t* out, int64_t out_len, void* workspace,
                      size_t workspace_bytes, void* stream) {
  const int64_t V = num_nodes, M = num_messages;
  const int32_t L = num_edge_types, D = num_levels;
  if (V < 0 || M < 0 || L < 1 || D < 0 || D > kMaxLevels || out_len < 0 || max_rows < 0 || max_messages < 0) return RELGNN_EINVAL;
  if (V * L >= INT32_MAX || M >= INT32_MAX || max_rows > V * L + 1 || max_messages > M) return RELGNN_EINVAL;
  if (D == 0) return RELGNN_OK;
  if (!desc || !rowptr_t || !rowptr_s || (out_len > 0 && !out)) return RELGNN_EINVAL;
  if (M > 0 && (!col_t || !perm_t || !inv_perm_t || !tgt_s || !frow_s || !pos_t_of_s || !perm_s)) return RELGNN_EINVAL;
  if (M > 0 && (!workspace || workspace_bytes < relgnn_level_plan_workspace_bytes(M, D))) return RELGNN_EINVAL;
  hipStream_t st = as_stream(stream);
  const int64_t stride = desc_stride(L), tiles = tiles_of(M);
  Workspace w = {nullptr, nullptr, nullptr};
  if (M > 0) {
    w = carve(workspace, M, D);
    flag_kernel<<<(unsigned)tiles, kTile, 0, st>>>(tgt_s, M, desc, stride, D, w);
    scan_kernel<<<1, kTile, 0, st>>>(tiles, D, w);
    compact_kernel<<<(unsigned)tiles, kTile, 0, st>>>(tgt_s, frow_s, pos_t_of_s, perm_s, M, L, desc, stride, D, w, out, out_len);
  }
  if (max_rows > 0)
    rowptr_kernel<<<flat_grid(max_rows, 256), 256, 0, st>>>(rowptr_t, rowptr_s, V * L + 1, M, L, desc, stride, D, max_rows, w, out, out_len);
  if (max_messages > 0)
    by_target_kernel<<<flat_grid(max_messages, 256), 256, 0, st>>>(col_t, perm_t, inv_perm_t, M, L, desc, stride, D, max_messages, out,
                                                                  out_len);
  return launch_status();
}

}  // extern "C"
