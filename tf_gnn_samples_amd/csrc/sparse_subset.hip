// A row subset of sparse node features, built on the device (include/relgnn_sparse_subset.h states the rule; tasks/sparse_features.py
// SparseRows.take_rows drives the two steps): the CSR of the rows a sampled batch names, the CSR of its transpose, the long-row plans.
//
// Count step — nothing here is sized by the subset's nnz:
//   sub_rowptr     a saturating exclusive scan of the named rows' lengths, read through a transform iterator (no length array)
//   sub_rowptr_t   one wave per named row adds 1 to the counter of each of its words (integer atomics: order-free), then a scan.
//                  (Measured at 98.7 k rows / 2.3 M entries: these adds are most of the count step.  A variant that lets the lanes
//                  of a wave agree on a word by ballot and add their number at once was slower, 2.07 against 1.50 ms: few rows
//                  share a word at the same position.  DESIGN.md section 7.4.)
//   plan offsets   per row (slabs, workspace rows, combos) in one scan of a three-counter item, again through a transform iterator,
//                  once per structure; the closing item of each scan is the total
//   sizes          one thread gathers the eight totals for the caller's one read-back
// Fill step: a wave per named row copies its entries; rocPRIM's stable radix sort orders the entry indices by column (keys: the
// subset's columns, values: a counting iterator), one gather writes (local row, value) — the local row of an entry by at most 32
// halvings over sub_rowptr; a thread per long row writes its slabs and its combo.
// Every store is checked against a capacity the host passed; no float atomics; no hand-over between workgroups.
#include "common.h"
#include "../../include/relgnn_sparse_features.h"
#include "../../include/relgnn_sparse_subset.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

using namespace relgnn;

namespace {

constexpr int64_t kIndexLimit = INT32_MAX;      // nnz, rows and columns stay below 2^31 - 1 (the container's own limit)

inline int key_bits(int64_t num_keys) {
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < num_keys) ++bits;
  return bits;
}

// min(a + b, 2^31 - 1) on non-negative counts: associative, so a scan may use it
struct SaturatingPlus {
  __host__ __device__ __forceinline__ int32_t operator()(int32_t a, int32_t b) const {
    const int64_t s = (int64_t)a + b;
    return s > kIndexLimit ? (int32_t)kIndexLimit : (int32_t)s;
  }
};

__device__ __forceinline__ int32_t row_length(const int32_t* __restrict__ rowptr, int64_t num_rows, int32_t v) {
  if ((uint32_t)v >= (uint64_t)num_rows) return 0;      // (validated by the caller; an id outside the matrix is an empty row)
  const int32_t len = rowptr[v + 1] - rowptr[v];
  return len > 0 ? len : 0;
}

// item i of the length scan: the length of source row nodes[i], 0 in the closing item
struct NamedRowLength {
  const int32_t* rowptr;
  const int32_t* nodes;
  int64_t num_rows, n;
  __device__ __forceinline__ int32_t operator()(int64_t i) const { return i < n ? row_length(rowptr, num_rows, nodes[i]) : 0; }
};

// what a row adds to the plan: its slabs, its workspace rows, 1 if it has a combo
struct PlanItem { int32_t slabs, ws, combos, pad; };

struct PlanPlus {
  __host__ __device__ __forceinline__ PlanItem operator()(const PlanItem& a, const PlanItem& b) const {
    return {a.slabs + b.slabs, a.ws + b.ws, a.combos + b.combos, 0};
  }
};

__device__ __forceinline__ int32_t slabs_of(int32_t len, int32_t split_above, int32_t slab) {
  return len > split_above ? (int32_t)(((int64_t)len + slab - 1) / slab) : 0;
}

struct PlanOfRow {
  const int32_t* rowptr;
  int64_t num_rows;
  int32_t split_above, slab;
  __device__ __forceinline__ PlanItem operator()(int64_t r) const {
    if (r >= num_rows) return {0, 0, 0, 0};
    const int32_t per_row = slabs_of(rowptr[r + 1] - rowptr[r], split_above, slab);
    return {per_row, per_row > 1 ? per_row : 0, per_row > 1 ? 1 : 0, 0};
  }
};

__global__ __launch_bounds__(256) void word_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         int64_t num_rows, int64_t num_cols, const int32_t* __restrict__ nodes,
                                                         int64_t n, int32_t* __restrict__ counts) {
  // one wave per named row, one add per entry (a row's words are distinct: no two lanes of a wave meet on a counter)
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  for (int64_t i = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + threadIdx.x / RELGNN_WAVE; i < n; i += waves) {
    const int32_t v = nodes[i], len = row_length(rowptr, num_rows, v);
    if (len == 0) continue;
    const int32_t* __restrict__ words = col + rowptr[v];
    for (int32_t j = lane; j < len; j += RELGNN_WAVE) {
      const int32_t f = words[j];
      if ((uint32_t)f < (uint64_t)num_cols) atomicAdd(counts + f, 1);
    }
  }
}

__global__ __launch_bounds__(64) void plan_sizes_kernel(const PlanItem* __restrict__ total, int32_t* __restrict__ sizes) {
  if (threadIdx.x == 0) {
    sizes[0] = total->slabs;
    sizes[1] = total->combos;
    sizes[2] = total->ws;
  }
}

__global__ __launch_bounds__(64) void subset_sizes_kernel(const int32_t* __restrict__ nnz, const PlanItem* __restrict__ rows,
                                                          const PlanItem* __restrict__ transposed, int32_t* __restrict__ sizes) {
  if (threadIdx.x == 0) {
    sizes[0] = *nnz;
    sizes[1] = rows->slabs, sizes[2] = rows->combos, sizes[3] = rows->ws;
    sizes[4] = transposed->slabs, sizes[5] = transposed->combos, sizes[6] = transposed->ws;
    sizes[7] = 0;
  }
}

__global__ __launch_bounds__(256) void plan_fill_kernel(const int32_t* __restrict__ rowptr, int64_t num_rows,
                                                        const PlanItem* __restrict__ offsets, int32_t split_above, int32_t slab,
                                                        int4* __restrict__ slabs, int64_t num_slabs, int32_t* __restrict__ combos,
                                                        int64_t num_combos) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < num_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t begin = rowptr[r], end = rowptr[r + 1];
    const int32_t per_row = slabs_of(end - begin, split_above, slab);
    if (per_row == 0) continue;
    const PlanItem at = offsets[r];
    for (int32_t s = 0; s < per_row; ++s) {
      const int64_t first = (int64_t)begin + (int64_t)s * slab, slot = (int64_t)at.slabs + s;
      const int64_t last = first + slab < end ? first + slab : end;
      if (slot >= 0 && slot < num_slabs) slabs[slot] = make_int4((int32_t)r, (int32_t)first, (int32_t)last, per_row > 1 ? at.ws + s : -1);
    }
    if (per_row > 1 && at.combos >= 0 && at.combos < num_combos) {
      int32_t* __restrict__ c = combos + (int64_t)at.combos * 3;
      c[0] = (int32_t)r, c[1] = at.ws, c[2] = per_row;
    }
  }
}

__global__ __launch_bounds__(256) void copy_rows_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        const float* __restrict__ val, int64_t num_rows,
                                                        const int32_t* __restrict__ nodes, int64_t n,
                                                        const int32_t* __restrict__ sub_rowptr, int64_t nnz,
                                                        int32_t* __restrict__ sub_col, float* __restrict__ sub_val) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / RELGNN_WAVE);
  for (int64_t i = blockIdx.x * (int64_t)(blockDim.x / RELGNN_WAVE) + threadIdx.x / RELGNN_WAVE; i < n; i += waves) {
    const int32_t v = nodes[i], len = row_length(rowptr, num_rows, v);
    if (len == 0) continue;
    const int64_t from = rowptr[v], to = sub_rowptr[i];
    for (int32_t j = lane; j < len; j += RELGNN_WAVE) {
      const int64_t slot = to + j;
      if (slot >= 0 && slot < nnz) {
        sub_col[slot] = col[from + j];
        sub_val[slot] = val[from + j];
      }
    }
  }
}

// the local row of entry j: the last i in [0, n) with sub_rowptr[i] <= j (rows without entries are stepped over); 32 halvings at most
__device__ __forceinline__ int32_t local_row(const int32_t* __restrict__ sub_rowptr, int64_t n, int64_t j) {
  int64_t lo = 0, hi = n;                                // first i in [0, n] with sub_rowptr[i] > j
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (sub_rowptr[mid] <= j) lo = mid + 1; else hi = mid;
  }
  return (int32_t)(lo > 0 ? lo - 1 : 0);
}

__global__ __launch_bounds__(256) void transpose_gather_kernel(const int32_t* __restrict__ order, int64_t nnz,
                                                               const int32_t* __restrict__ sub_rowptr, int64_t n,
                                                               const float* __restrict__ sub_val, int32_t* __restrict__ sub_col_t,
                                                               float* __restrict__ sub_val_t) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = order[e];
    if (j < 0 || j >= nnz) continue;                     // (a permutation of [0, nnz): never taken)
    sub_col_t[e] = local_row(sub_rowptr, n, j);
    sub_val_t[e] = sub_val[j];
  }
}

size_t plan_scan_temp_bytes(int64_t items) {
  size_t bytes = 0;
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), PlanOfRow{nullptr, 0, 0, 0});
  rocprim::exclusive_scan(nullptr, bytes, in, static_cast<PlanItem*>(nullptr), PlanItem{0, 0, 0, 0}, (size_t)items, PlanPlus(),
                          (hipStream_t)0);
  return bytes;
}

size_t count_scan_temp_bytes(int64_t items) {
  size_t named = 0, plain = 0;
  int32_t* p = nullptr;
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), NamedRowLength{nullptr, nullptr, 0, 0});
  rocprim::exclusive_scan(nullptr, named, in, p, (int32_t)0, (size_t)items, SaturatingPlus(), (hipStream_t)0);
  rocprim::exclusive_scan(nullptr, plain, p, p, (int32_t)0, (size_t)items, SaturatingPlus(), (hipStream_t)0);
  return named > plain ? named : plain;
}

inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// offsets [num_rows + 1] of one row-pointer array; the closing item is the total
int plan_offsets(const int32_t* rowptr, int64_t num_rows, PlanItem* offsets, void* temp, size_t temp_bytes, hipStream_t st) {
  const PlanOfRow item{rowptr, num_rows, (int32_t)relgnn_csr_project_split_above(), (int32_t)relgnn_csr_project_slab()};
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), item);
  if (rocprim::exclusive_scan(temp, temp_bytes, in, offsets, PlanItem{0, 0, 0, 0}, (size_t)(num_rows + 1), PlanPlus(), st) != hipSuccess)
    return RELGNN_EHIP;
  return RELGNN_OK;
}

}  // namespace

extern "C" {

int relgnn_sparse_subset_supported(int64_t num_rows, int64_t num_cols, int64_t n) {
  return num_rows >= 0 && num_cols >= 0 && n >= 0 && num_rows < kIndexLimit && num_cols < kIndexLimit && n < kIndexLimit ? 1 : 0;
}

size_t relgnn_split_plan_workspace_bytes(int64_t num_rows) {
  if (num_rows < 0) num_rows = 0;
  return align_up(plan_scan_temp_bytes(num_rows + 1), 256) + 256;
}

int relgnn_split_plan_count(const int32_t* rowptr, int64_t num_rows, int32_t* offsets, int32_t* sizes, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (num_rows < 0 || !rowptr || !offsets || !sizes || !workspace) return RELGNN_EINVAL;
  if (num_rows >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(offsets) & 15u) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_split_plan_workspace_bytes(num_rows)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  PlanItem* items = reinterpret_cast<PlanItem*>(offsets);
  const int status = plan_offsets(rowptr, num_rows, items, workspace, workspace_bytes, st);
  if (status != RELGNN_OK) return status;
  plan_sizes_kernel<<<1, 64, 0, st>>>(items + num_rows, sizes);
  return launch_status();
}

int relgnn_split_plan_fill(const int32_t* rowptr, int64_t num_rows, const int32_t* offsets, int32_t* slabs, int64_t num_slabs,
                           int32_t* combos, int64_t num_combos, void* stream) {
  if (num_rows < 0 || num_slabs < 0 || num_combos < 0) return RELGNN_EINVAL;
  if (num_rows >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (num_rows == 0 || num_slabs == 0) return RELGNN_OK;                  // (no long row: no combo either)
  if (!rowptr || !offsets || !slabs || (num_combos > 0 && !combos)) return RELGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(slabs)) & 15u) return RELGNN_EINVAL;
  plan_fill_kernel<<<flat_grid(num_rows, 256), 256, 0, as_stream(stream)>>>(
      rowptr, num_rows, reinterpret_cast<const PlanItem*>(offsets), (int32_t)relgnn_csr_project_split_above(),
      (int32_t)relgnn_csr_project_slab(), reinterpret_cast<int4*>(slabs), num_slabs, combos, num_combos);
  return launch_status();
}

size_t relgnn_sparse_subset_count_workspace_bytes(int64_t n, int64_t num_cols) {
  if (n < 0) n = 0;
  if (num_cols < 0) num_cols = 0;
  // [per-word counters: num_cols + 1 int32 | rocPRIM's scan storage, the largest of the four scans']
  const size_t of_rows = max3(count_scan_temp_bytes(n + 1), plan_scan_temp_bytes(n + 1), 0);
  const size_t of_words = max3(count_scan_temp_bytes(num_cols + 1), plan_scan_temp_bytes(num_cols + 1), 0);
  return align_up((size_t)(num_cols + 1) * 4, 256) + align_up(max3(of_rows, of_words, 0), 256) + 256;
}

int relgnn_sparse_subset_count(const int32_t* rowptr, const int32_t* col, int64_t num_rows, int64_t num_cols, const int32_t* nodes,
                               int64_t n, int32_t* sub_rowptr, int32_t* sub_rowptr_t, int32_t* plan_offsets_rows,
                               int32_t* plan_offsets_t, int32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!relgnn_sparse_subset_supported(num_rows, num_cols, n)) return num_rows < 0 || num_cols < 0 || n < 0 ? RELGNN_EINVAL : RELGNN_EUNSUPPORTED;
  if (!rowptr || !sub_rowptr || !sub_rowptr_t || !plan_offsets_rows || !plan_offsets_t || !sizes || !workspace) return RELGNN_EINVAL;
  if (n > 0 && !nodes) return RELGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(plan_offsets_rows) | reinterpret_cast<uintptr_t>(plan_offsets_t)) & 15u) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_sparse_subset_count_workspace_bytes(n, num_cols)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  int32_t* counts = static_cast<int32_t*>(workspace);
  const size_t front = align_up((size_t)(num_cols + 1) * 4, 256);
  void* temp = static_cast<char*>(workspace) + front;
  const size_t temp_bytes = workspace_bytes - front;

  size_t bytes = temp_bytes;
  auto lengths = rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), NamedRowLength{rowptr, nodes, num_rows, n});
  if (rocprim::exclusive_scan(temp, bytes, lengths, sub_rowptr, (int32_t)0, (size_t)(n + 1), SaturatingPlus(), st) != hipSuccess)
    return RELGNN_EHIP;

  if (hipMemsetAsync(counts, 0, (size_t)(num_cols + 1) * 4, st) != hipSuccess) return RELGNN_EHIP;
  if (n > 0 && col) word_count_kernel<<<flat_grid(n * RELGNN_WAVE, 256), 256, 0, st>>>(rowptr, col, num_rows, num_cols, nodes, n, counts);
  bytes = temp_bytes;
  if (rocprim::exclusive_scan(temp, bytes, counts, sub_rowptr_t, (int32_t)0, (size_t)(num_cols + 1), SaturatingPlus(), st) != hipSuccess)
    return RELGNN_EHIP;

  PlanItem* of_rows = reinterpret_cast<PlanItem*>(plan_offsets_rows);
  PlanItem* of_t = reinterpret_cast<PlanItem*>(plan_offsets_t);
  int status = plan_offsets(sub_rowptr, n, of_rows, temp, temp_bytes, st);
  if (status == RELGNN_OK) status = plan_offsets(sub_rowptr_t, num_cols, of_t, temp, temp_bytes, st);
  if (status != RELGNN_OK) return status;
  subset_sizes_kernel<<<1, 64, 0, st>>>(sub_rowptr + n, of_rows + n, of_t + num_cols, sizes);
  return launch_status();
}

int relgnn_sparse_subset_copy(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows, const int32_t* nodes,
                              int64_t n, const int32_t* sub_rowptr, int64_t nnz, int32_t* sub_col, float* sub_val, void* stream) {
  if (num_rows < 0 || n < 0 || nnz < 0 || nnz >= kIndexLimit) return RELGNN_EINVAL;
  if (num_rows >= kIndexLimit || n >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (n == 0 || nnz == 0) return RELGNN_OK;
  if (!rowptr || !col || !val || !nodes || !sub_rowptr || !sub_col || !sub_val) return RELGNN_EINVAL;
  copy_rows_kernel<<<flat_grid(n * RELGNN_WAVE, 256), 256, 0, as_stream(stream)>>>(rowptr, col, val, num_rows, nodes, n, sub_rowptr, nnz,
                                                                                   sub_col, sub_val);
  return launch_status();
}

size_t relgnn_sparse_subset_transpose_workspace_bytes(int64_t nnz, int64_t num_cols) {
  if (nnz <= 0) return 256;
  size_t temp = 0;
  int32_t* p = nullptr;
  rocprim::radix_sort_pairs(nullptr, temp, p, p, rocprim::counting_iterator<int32_t>(0), p, (size_t)nnz, 0, key_bits(num_cols), (hipStream_t)0);
  // [sorted columns | entry order | rocPRIM's sort storage]
  return align_up((size_t)nnz * 4, 256) * 2 + align_up(temp, 256) + 256;
}

int relgnn_sparse_subset_transpose(const int32_t* sub_rowptr, int64_t n, const int32_t* sub_col, const float* sub_val, int64_t nnz,
                                   int64_t num_cols, int32_t* sub_col_t, float* sub_val_t, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (n < 0 || nnz < 0 || num_cols < 0 || nnz >= kIndexLimit) return RELGNN_EINVAL;
  if (n >= kIndexLimit || num_cols >= kIndexLimit) return RELGNN_EUNSUPPORTED;
  if (nnz == 0) return RELGNN_OK;
  if (n == 0 || !sub_rowptr || !sub_col || !sub_val || !sub_col_t || !sub_val_t || !workspace) return RELGNN_EINVAL;
  if (workspace_bytes < relgnn_sparse_subset_transpose_workspace_bytes(nnz, num_cols)) return RELGNN_ENOSPC;
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  const size_t seg = align_up((size_t)nnz * 4, 256);
  int32_t* sorted_cols = reinterpret_cast<int32_t*>(ws);
  int32_t* order = reinterpret_cast<int32_t*>(ws + seg);
  size_t temp_bytes = workspace_bytes - 2 * seg;
  // stable: the entries of a column keep their order, which is ascending local row
  if (rocprim::radix_sort_pairs(ws + 2 * seg, temp_bytes, sub_col, sorted_cols, rocprim::counting_iterator<int32_t>(0), order, (size_t)nnz,
                                0, key_bits(num_cols), st) != hipSuccess)
    return RELGNN_EHIP;
  transpose_gather_kernel<<<flat_grid(nnz, 256), 256, 0, st>>>(order, nnz, sub_rowptr, n, sub_val, sub_col_t, sub_val_t);
  return launch_status();
}

}  // extern "C"
