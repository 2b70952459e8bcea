// QM9 readout head (tasks/qm9_task.py:163-197 of the reference), every regression task of a batch in one call:
//   out   = x_v . w_reg[t] + b_reg[t]                         Dense(1) over the final node states
//   gate  = sigmoid([x_v | a_v] . w_gate[t] + b_gate[t])      Dense(1) over [states | initial features]; the concatenation is never built
//   y[t, g] = sum over the graph's nodes of gate * out        tf.unsorted_segment_sum over graph_nodes_list
//   e = y - target;  abs_err[t] = sum_g |e|;  loss = sum_t mean_g 0.5 e^2;  total_loss = loss * G
// Deterministic: no float atomics; every sum has a fixed order.  A node's arithmetic is the same chain of operations whatever its row
// number, a graph's sum runs over its nodes counted from the graph's first node, and the backward's workgroups own fixed ranges of 256
// nodes: the same graph gives the same bits wherever it stands in the batch, and a task the same bits whatever its place in the list.
#include "common.h"

using namespace relgnn;

namespace {

constexpr int kMaxT = 16, kMaxHidden = 512, kMaxA = 64;
constexpr int kGroup = 16;                           // lanes that share one node: lane l takes the float4 chunks l, l + 16, ...
constexpr int kTile = 256;                           // nodes per workgroup of the backward: [kTile][2 * kMaxT] floats of LDS (32 KB)

// The T device pointers per variable family travel BY VALUE in the kernel arguments (512 bytes): nothing is stacked or uploaded.
struct HeadWeights {
  const float* w_reg[kMaxT];
  const float* b_reg[kMaxT];
  const float* w_gate[kMaxT];
  const float* b_gate[kMaxT];
};
struct HeadGrads {
  float* w_reg[kMaxT];
  float* b_reg[kMaxT];
  float* w_gate[kMaxT];
  float* b_gate[kMaxT];
};

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = kGroup / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ float sigmoidf(float z) {           // finite for every finite z: exp only of non-positive arguments
  const float e = expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) / (1.f + e);
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// First index whose id is not below `key`.  Every probe lies in [0, V): safe for ANY contents of ids.
__device__ __forceinline__ long long lower_bound_ids(const int* __restrict__ ids, long long V, long long key) {
  long long lo = 0, hi = V;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if ((long long)ids[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// o[t], z[t] = the two pre-activations of one node for every task, in all 16 lanes of the node's group.  x is read once, as float4.
__device__ __forceinline__ void node_dots(const float* __restrict__ x, const float* __restrict__ a, int hidden, int A,
                                          const HeadWeights& w, int T, int l, bool active, float (&o)[kMaxT], float (&z)[kMaxT]) {
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) o[t] = z[t] = 0.f;
  if (active) {
    for (int c = 4 * l; c < hidden; c += 4 * kGroup) {
      const float4 xv = *reinterpret_cast<const float4*>(x + c);
#pragma unroll
      for (int t = 0; t < kMaxT; ++t) {
        if (t < T) {
          o[t] = dot4(xv, *reinterpret_cast<const float4*>(w.w_reg[t] + c), o[t]);
          z[t] = dot4(xv, *reinterpret_cast<const float4*>(w.w_gate[t] + c), z[t]);
        }
      }
    }
    for (int j = l; j < A; j += kGroup) {
      const float av = a[j];
#pragma unroll
      for (int t = 0; t < kMaxT; ++t)
        if (t < T) z[t] = fmaf(av, w.w_gate[t][hidden + j], z[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < kMaxT; ++t) {
    if (t < T) {                                     // T is uniform: every lane takes part in the shuffles
      o[t] = group_sum(o[t]) + w.b_reg[t][0];
      z[t] = group_sum(z[t]) + w.b_gate[t][0];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: one wave per graph, four nodes at a time (16 lanes each); then every thread of the grid checks its share of the ids
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qm9_head_fwd_kernel(const float* __restrict__ X, long long ld, const float* __restrict__ F,
                                                           long long ldf, const int* __restrict__ ids, long long V, long long G,
                                                           int hidden, int A, int T, const HeadWeights w, float* __restrict__ y,
                                                           int* __restrict__ node_range, uint32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kGroup, l = lane % kGroup;
  const long long g = (long long)blockIdx.x * 4 + wave;
  if (g < G) {                                       // wave-uniform
    // the graph's node range in the non-decreasing list; on a list that breaks the contract: SOME range inside [0, V)
    const long long lo = lower_bound_ids(ids, V, g);
    long long hi = lower_bound_ids(ids, V, g + 1);
    if (hi < lo) hi = lo;
    float acc[kMaxT];
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) acc[t] = 0.f;
    for (long long v0 = lo; v0 < hi; v0 += 64 / kGroup) {
      const long long v = v0 + grp;
      const bool active = v < hi && (long long)ids[v] == g;       // a node with another id inside the range counts for nothing
      const long long row = active ? v : lo;
      float o[kMaxT], z[kMaxT];
      node_dots(X + row * ld, F + row * ldf, hidden, A, w, T, l, active, o, z);
#pragma unroll
      for (int t = 0; t < kMaxT; ++t)
        if (t < T) acc[t] += active ? sigmoidf(z[t]) * o[t] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
      if (t < T) {
        float s = acc[t];                            // nodes 0, 4, 8, ... of the graph in group 0, 1, 5, ... in group 1, ...
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (lane == 0) y[(long long)t * G + g] = s;  // an empty graph: 0, as unsorted_segment_sum gives
      }
    }
    if (lane == 0) {
      node_range[2 * g] = (int)lo;
      node_range[2 * g + 1] = (int)hi;
    }
  }
  // the contract of graph_nodes_list, checked pair by pair and independently of the searches above
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
    const int id = ids[v];
    uint32_t bad = 0;
    if (id < 0 || (long long)id >= G) bad |= RELGNN_ERRFLAG_INDEX_OUT_OF_RANGE;
    if (v > 0 && id < ids[v - 1]) bad |= RELGNN_ERRFLAG_NOT_SORTED;
    if (bad != 0 && err != nullptr) atomicOr(err, bad);
  }
}

// stats = [abs_err[0 .. T), loss, total_loss]: per task, thread i adds graphs i, i + 256, ... in double, then a fixed tree
__global__ __launch_bounds__(256) void qm9_head_stats_kernel(const float* __restrict__ y, const float* __restrict__ target, long long G,
                                                             int T, float* __restrict__ stats) {
  __shared__ double red[4][2];
  double loss = 0.0;
  for (int t = 0; t < T; ++t) {
    double a = 0.0, b = 0.0;
    for (long long g = threadIdx.x; g < G; g += 256) {
      const float e = y[(long long)t * G + g] - target[(long long)t * G + g];      // float32, as the reference subtracts
      a += fabs((double)e);
      b += 0.5 * ((double)e * (double)e);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off); b += __shfl_xor(b, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      stats[t] = (float)((red[0][0] + red[1][0]) + (red[2][0] + red[3][0]));
      loss += ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) / (double)G;     // tf.reduce_mean over the graphs (:192)
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[T] = (float)loss;
    stats[T + 1] = (float)loss * (float)G;           // metrics['loss'] * num_graphs, a float32 product
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: workgroup b owns the nodes [b * kTile, (b + 1) * kTile).
//   phase 1 (16 lanes per node): out and gate again, d out and d (gate pre-activation) of every task into LDS
//   phase 2 (one thread per column of [states | features | 1]): the node's input gradient, and down the tile's nodes in node order
//           the column's share of every weight and bias gradient, in double -> the workgroup's partial
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qm9_head_bwd_kernel(const float* __restrict__ X, long long ld, const float* __restrict__ F,
                                                           long long ldf, const int* __restrict__ ids, long long V, long long G,
                                                           int hidden, int A, int T, const HeadWeights w,
                                                           const float* __restrict__ target, const float* __restrict__ y,
                                                           const int* __restrict__ node_range, const float* __restrict__ g_loss,
                                                           const float* __restrict__ g_total, float* __restrict__ dX, long long ldg,
                                                           float* __restrict__ dF, double* __restrict__ partial) {
  __shared__ float4 sd[kTile][2 * kMaxT / 4];        // per node: d out [kMaxT], then d z [kMaxT]
  float* sdf = reinterpret_cast<float*>(&sd[0][0]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kGroup, l = lane % kGroup;
  const long long base = (long long)blockIdx.x * kTile;
  const int here = (int)(V - base < kTile ? V - base : kTile);
  // d loss / d y = e / G, d total_loss / d y = e
  float gs = 0.f;
  if (g_loss) gs = g_loss[0] / (float)G;
  if (g_total) gs = g_loss ? gs + g_total[0] : g_total[0];

  for (int n0 = 0; n0 < here; n0 += 16) {
    const int n = n0 + wave * 4 + grp;
    const long long v = base + n;
    const bool in = n < here;
    const long long gid = in ? (long long)ids[v] : -1;
    bool active = in && gid >= 0 && gid < G;
    if (active) active = (long long)node_range[2 * gid] <= v && v < (long long)node_range[2 * gid + 1];   // the forward's test
    const long long row = active ? v : base;
    float o[kMaxT], z[kMaxT];
    node_dots(X + row * ld, F + row * ldf, hidden, A, w, T, l, active, o, z);
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
      float d_out = 0.f, d_z = 0.f;
      if (t < T && active) {
        const float e = y[(long long)t * G + gid] - target[(long long)t * G + gid];
        const float de = gs * e, gate = sigmoidf(z[t]);
        d_out = de * gate;
        d_z = (de * o[t]) * (gate * (1.f - gate));
      }
      if (l == 0 && in) {
        sdf[n * 2 * kMaxT + t] = d_out;
        sdf[n * 2 * kMaxT + kMaxT + t] = d_z;
      }
    }
  }
  __syncthreads();

  const int ncols = hidden + A + 1;
  for (int c = threadIdx.x; c < ncols; c += 256) {
    const bool is_state = c < hidden, is_feature = !is_state && c < hidden + A;
    float wr[kMaxT], wg[kMaxT];
    double ar[kMaxT], ag[kMaxT];
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
      wr[t] = (t < T && is_state) ? w.w_reg[t][c] : 0.f;
      wg[t] = (t < T && (is_state || is_feature)) ? w.w_gate[t][c] : 0.f;
      ar[t] = ag[t] = 0.0;
    }
    for (int n = 0; n < here; ++n) {
      const long long v = base + n;
      const float xv = is_state ? X[v * ld + c] : (is_feature ? F[v * ldf + (c - hidden)] : 1.f);
      float dx = 0.f;
#pragma unroll
      for (int q = 0; q < kMaxT / 4; ++q) {
        if (4 * q < T) {
          const float4 po = sd[n][q], pz = sd[n][kMaxT / 4 + q];
          const float d_out[4] = {po.x, po.y, po.z, po.w}, d_z[4] = {pz.x, pz.y, pz.z, pz.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int t = 4 * q + k;
            if (t < T) {
              dx = fmaf(d_z[k], wg[t], fmaf(d_out[k], wr[t], dx));
              ar[t] = fma((double)d_out[k], (double)xv, ar[t]);
              ag[t] = fma((double)d_z[k], (double)xv, ag[t]);
            }
          }
        }
      }
      if (is_state) dX[v * ldg + c] = dx;
      else if (is_feature && dF != nullptr) dF[v * A + (c - hidden)] = dx;
    }
    double* mine = partial + (long long)blockIdx.x * (2 * T * ncols);
#pragma unroll
    for (int t = 0; t < kMaxT; ++t) {
      if (t < T) {
        mine[(2 * t) * ncols + c] = ar[t];
        mine[(2 * t + 1) * ncols + c] = ag[t];
      }
    }
  }
}

// Element e = (task, family, column) of the partials: the workgroups' shares in workgroup order (four contiguous quarters, one per
// wave, then the quarters in order), rounded once to float32 and written into that variable's own gradient buffer.
__global__ __launch_bounds__(256) void qm9_head_combine_kernel(const double* __restrict__ partial, int nblk, int T, int hidden, int A,
                                                               const HeadGrads grads) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncols = hidden + A + 1, n_el = 2 * T * ncols;
  const int e = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (e < n_el) {
    const int per = (nblk + 3) / 4;
    const int b1 = (wave + 1) * per < nblk ? (wave + 1) * per : nblk;
    for (int b = wave * per; b < b1; ++b) s += partial[(long long)b * n_el + e];
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || e >= n_el) return;
  const float total = (float)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
  const int t = e / (2 * ncols), r = e - t * 2 * ncols;
  const bool gate = r >= ncols;
  const int c = gate ? r - ncols : r;
  float* dst = nullptr;
#pragma unroll
  for (int u = 0; u < kMaxT; ++u) {
    if (u == t) {
      if (c == hidden + A) dst = gate ? grads.b_gate[u] : grads.b_reg[u];
      else if (gate) dst = grads.w_gate[u] + c;
      else if (c < hidden) dst = grads.w_reg[u] + c;              // (the regression product has no feature columns)
    }
  }
  if (dst != nullptr) *dst = total;
}

static inline bool qm9_head_shape_ok(int32_t T, int32_t hidden, int32_t A) {
  return T >= 1 && T <= kMaxT && hidden >= 4 && hidden <= kMaxHidden && hidden % 4 == 0 && A >= 1 && A <= kMaxA;
}

static inline long long bwd_blocks(long long V) { return (V + kTile - 1) / kTile; }

}  // namespace

extern "C" {

int relgnn_qm9_head_supported(int32_t num_tasks, int32_t hidden, int32_t annotation_size) {
  return qm9_head_shape_ok(num_tasks, hidden, annotation_size) ? 1 : 0;
}

size_t relgnn_qm9_head_workspace_bytes(int64_t num_nodes, int32_t num_tasks, int32_t hidden, int32_t annotation_size) {
  if (num_nodes <= 0 || !qm9_head_shape_ok(num_tasks, hidden, annotation_size)) return 256;
  return (size_t)bwd_blocks(num_nodes) * 2 * (size_t)num_tasks * (size_t)(hidden + annotation_size + 1) * sizeof(double);
}

int relgnn_qm9_head_fwd(const float* states, int64_t ld, const float* features, int64_t ldf, const int32_t* graph_nodes_list,
                        int64_t num_nodes, int64_t num_graphs, int32_t hidden, int32_t annotation_size, int32_t num_tasks,
                        const float* const* w_reg, const float* const* b_reg, const float* const* w_gate, const float* const* b_gate,
                        const float* targets, float* y, int32_t* node_range, float* stats, uint32_t* err_flag, void* stream) {
  if (!qm9_head_shape_ok(num_tasks, hidden, annotation_size)) return RELGNN_EUNSUPPORTED;
  if (num_nodes < 0 || num_nodes > INT32_MAX || num_graphs < 1 || num_graphs > INT32_MAX) return RELGNN_EINVAL;
  if (ld < hidden || ld % 4 != 0 || ldf < annotation_size) return RELGNN_EINVAL;
  if (!w_reg || !b_reg || !w_gate || !b_gate || !targets || !y || !node_range || !stats) return RELGNN_EINVAL;
  if (num_nodes > 0 && (!states || !features || !graph_nodes_list || !aligned16(states))) return RELGNN_EINVAL;
  HeadWeights w = {};
  for (int t = 0; t < num_tasks; ++t) {
    if (!w_reg[t] || !b_reg[t] || !w_gate[t] || !b_gate[t] || !aligned16(w_reg[t]) || !aligned16(w_gate[t])) return RELGNN_EINVAL;
    w.w_reg[t] = w_reg[t]; w.b_reg[t] = b_reg[t]; w.w_gate[t] = w_gate[t]; w.b_gate[t] = b_gate[t];
  }
  hipStream_t st = as_stream(stream);
  qm9_head_fwd_kernel<<<(unsigned)((num_graphs + 3) / 4), 256, 0, st>>>(states, ld, features, ldf, graph_nodes_list, num_nodes, num_graphs,
                                                                       hidden, annotation_size, num_tasks, w, y, node_range, err_flag);
  qm9_head_stats_kernel<<<1, 256, 0, st>>>(y, targets, num_graphs, num_tasks, stats);
  return launch_status();
}

int relgnn_qm9_head_bwd(const float* states, int64_t ld, const float* features, int64_t ldf, const int32_t* graph_nodes_list,
                        int64_t num_nodes, int64_t num_graphs, int32_t hidden, int32_t annotation_size, int32_t num_tasks,
                        const float* const* w_reg, const float* const* b_reg, const float* const* w_gate, const float* const* b_gate,
                        const float* targets, const float* y, const int32_t* node_range, const float* g_loss, const float* g_total,
                        float* d_states, int64_t ldg, float* d_features, float* const* d_w_reg, float* const* d_b_reg,
                        float* const* d_w_gate, float* const* d_b_gate, void* workspace, size_t workspace_bytes, void* stream) {
  if (!qm9_head_shape_ok(num_tasks, hidden, annotation_size)) return RELGNN_EUNSUPPORTED;
  if (num_nodes < 0 || num_nodes > INT32_MAX || num_graphs < 1 || num_graphs > INT32_MAX) return RELGNN_EINVAL;
  if (ld < hidden || ld % 4 != 0 || ldf < annotation_size || ldg < hidden) return RELGNN_EINVAL;
  if (!w_reg || !b_reg || !w_gate || !b_gate || !d_w_reg || !d_b_reg || !d_w_gate || !d_b_gate) return RELGNN_EINVAL;
  if (!targets || !y || !node_range || (!g_loss && !g_total)) return RELGNN_EINVAL;
  if (num_nodes > 0 && (!states || !features || !graph_nodes_list || !d_states || !aligned16(states))) return RELGNN_EINVAL;
  if (!workspace || workspace_bytes < relgnn_qm9_head_workspace_bytes(num_nodes, num_tasks, hidden, annotation_size)) return RELGNN_ENOSPC;
  HeadWeights w = {};
  HeadGrads g = {};
  for (int t = 0; t < num_tasks; ++t) {
    if (!w_reg[t] || !b_reg[t] || !w_gate[t] || !b_gate[t] || !aligned16(w_reg[t]) || !aligned16(w_gate[t])) return RELGNN_EINVAL;
    if (!d_w_reg[t] || !d_b_reg[t] || !d_w_gate[t] || !d_b_gate[t]) return RELGNN_EINVAL;
    w.w_reg[t] = w_reg[t]; w.b_reg[t] = b_reg[t]; w.w_gate[t] = w_gate[t]; w.b_gate[t] = b_gate[t];
    g.w_reg[t] = d_w_reg[t]; g.b_reg[t] = d_b_reg[t]; g.w_gate[t] = d_w_gate[t]; g.b_gate[t] = d_b_gate[t];
  }
  hipStream_t st = as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  const int nblk = (int)bwd_blocks(num_nodes);
  if (nblk > 0)
    qm9_head_bwd_kernel<<<nblk, 256, 0, st>>>(states, ld, features, ldf, graph_nodes_list, num_nodes, num_graphs, hidden, annotation_size,
                                              num_tasks, w, targets, y, node_range, g_loss, g_total, d_states, ldg, d_features, partial);
  const int n_el = 2 * num_tasks * (hidden + annotation_size + 1);
  qm9_head_combine_kernel<<<(n_el + 63) / 64, 256, 0, st>>>(partial, nblk, num_tasks, hidden, annotation_size, g);      // nblk == 0: zeros
  return launch_status();
}

}  // extern "C"
