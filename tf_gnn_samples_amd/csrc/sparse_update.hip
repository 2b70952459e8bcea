// Row-deferred Adam (include/relgnn_sparse_update.h): dense Adam's bits for a [F, n] row table while a step touches only the rows
// its batch names.  A row outside the batch has a gradient of +0 and is not read by the forward; its missed steps are replayed
// through the dense launch's own element function (adam_element.h) with g = +0 before it is read again.
//
// Streaming kernels: per named row 3 (catch-up) or 4 (step) arrays of n floats are read and 3 written, 16 bytes per lane, a row's
// n floats contiguous.  A wave takes 64 consecutive rows: lane l reads the rowptr_t pair and the stamp of row 64 c + l (two coalesced
// 256-byte reads and, for named rows, a third), the ballot of "has work" is the wave's to-do list, and the wave walks it row by row.
// The compact step (relgnn_rows_adam_step_compact) walks a list of named words instead: 64 list entries per wave, no row pointer.
// One wave per ROW would make a 2^20-row table 2^20 mostly empty waves; this way an unnamed row costs 8 bytes of one read.
#include "common.h"
#include "adam_element.h"
#include "../../include/relgnn_sparse_update.h"
#include "../../include/relgnn_sparse_gradient.h"

using namespace relgnn;

namespace {

constexpr int kBlock = 256;            // four waves, each on 64 rows of its own
constexpr int kMaxBlocks = 256 * 8;    // flat_grid's cap: the waves stride over the rest

__device__ __forceinline__ void adam_element4(float4& p, const float4& gi, float4& m, float4& v, float lr_t, float b1, float b2,
                                              float eps) {
  adam_element(p.x, gi.x, m.x, v.x, lr_t, b1, b2, eps);
  adam_element(p.y, gi.y, m.y, v.y, lr_t, b1, b2, eps);
  adam_element(p.z, gi.z, m.z, v.z, lr_t, b1, b2, eps);
  adam_element(p.w, gi.w, m.w, v.w, lr_t, b1, b2, eps);
}

// STEP = false: named rows behind t replay steps stamp + 1 .. t.
// STEP = true : named rows replay steps stamp + 1 .. t - 1, then take step t with g * scale and lr_t; step_sizes[t - base - 1] = lr_t
//               (the replays read entries below that one only).
// COMPACT (include/relgnn_sparse_gradient.h): F counts the named rows, which are words[0 .. F), each in [0, table_rows), and the
//               gradient row of words[i] is g row i.  Otherwise rows 0 .. F of the table are walked and row f's gradient is g row f.
// n4 = n / 4; ld and ld_g in floats, multiples of 4.  Every loop is bounded by F, n4 and t - base.
template <bool STEP, bool COMPACT>
__global__ __launch_bounds__(kBlock) void rows_adam_kernel(const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ words,
                                                           long long table_rows, long long F, float* __restrict__ p,
                                                           const float* __restrict__ g, long long ld_g, float* __restrict__ m,
                                                           float* __restrict__ v, long long ld, int n4, int32_t* __restrict__ stamps,
                                                           float* step_sizes, int base, int t, const float* __restrict__ norm,
                                                           float clip, float lr_t, float b1, float b2, float eps) {
  const int lane = threadIdx.x & (RELGNN_WAVE - 1);
  const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) / RELGNN_WAVE;
  const long long num_waves = (long long)gridDim.x * kBlock / RELGNN_WAVE;
  float scale = 1.f;
  if (STEP) {
    if (clip > 0.f) scale = clip / fmaxf(norm[0], clip);      // (mt_adam_clip_kernel's expression)
    if (blockIdx.x == 0 && threadIdx.x == 0) step_sizes[t - base - 1] = lr_t;
  }
  const int replay_to = STEP ? t - 1 : t;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long chunks = (F + RELGNN_WAVE - 1) / RELGNN_WAVE;
  for (long long chunk = wave; chunk < chunks; chunk += num_waves) {
    long long f = chunk * RELGNN_WAVE + lane;
    bool work = false, named = false;
    int stamp = 0;
    if (COMPACT) {
      if (f < F) {
        f = words[f];
        named = f >= 0 && f < table_rows;
      }
    } else {
      named = f < F && (!rowptr_t || rowptr_t[f + 1] > rowptr_t[f]);
    }
    if (named) {
      stamp = max(stamps[f], base);                           // (a stamp below base: the loop is clamped to the table)
      work = STEP || stamp < replay_to;
    }
    unsigned long long todo = __ballot(work);
    while (todo) {                                            // the same word in every lane: the wave stays together
      const int l = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int from = __builtin_amdgcn_readfirstlane(__shfl(stamp, l));
      const long long g_row = chunk * RELGNN_WAVE + l;
      long long row = g_row;
      if (COMPACT) row = __builtin_amdgcn_readfirstlane(__shfl((int)f, l));
      float4* p4 = reinterpret_cast<float4*>(p + row * ld);
      float4* m4 = reinterpret_cast<float4*>(m + row * ld);
      float4* v4 = reinterpret_cast<float4*>(v + row * ld);
      for (int c = lane; c < n4; c += RELGNN_WAVE) {
        float4 pv = p4[c], mv = m4[c], vv = v4[c], gv = zero;
        if (STEP) {
          gv = reinterpret_cast<const float4*>(g + g_row * ld_g)[c];
          gv.x = gv.x * scale; gv.y = gv.y * scale; gv.z = gv.z * scale; gv.w = gv.w * scale;
        }
        for (int step = from + 1; step <= replay_to; ++step)
          adam_element4(pv, zero, mv, vv, step_sizes[step - base - 1], b1, b2, eps);
        if (STEP) adam_element4(pv, gv, mv, vv, lr_t, b1, b2, eps);
        m4[c] = mv;
        v4[c] = vv;
        p4[c] = pv;
      }
    }
    if (work) stamps[f] = t;
  }
}

static inline unsigned rows_grid(int64_t F) {
  const int64_t chunks = (F + RELGNN_WAVE - 1) / RELGNN_WAVE;
  const int64_t per_block = kBlock / RELGNN_WAVE;
  int64_t blocks = (chunks + per_block - 1) / per_block;
  if (blocks < 1) blocks = 1;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  return (unsigned)blocks;
}

static inline bool rows_ok(const void* a, int64_t ld, int32_t n) { return a && aligned16(a) && ld >= n && ld % 4 == 0; }

}  // namespace

extern "C" {

int relgnn_rows_adam_supported(int32_t n) { return n >= 4 && n <= 1024 && n % 4 == 0; }

int relgnn_rows_adam_catch_up(const int32_t* rowptr_t, int64_t F, float* p, float* m, float* v, int64_t ld, int32_t n,
                              int32_t* stamps, const float* step_sizes, int32_t base, int32_t t_now, float beta1, float beta2,
                              float eps, void* stream) {
  if (F < 0 || F >= INT32_MAX || base < 0 || t_now < base) return RELGNN_EINVAL;
  if (!relgnn_rows_adam_supported(n)) return RELGNN_EUNSUPPORTED;
  if (F == 0 || t_now == base) return RELGNN_OK;              // no stamp is below base: nothing is behind
  if (!rows_ok(p, ld, n) || !rows_ok(m, ld, n) || !rows_ok(v, ld, n) || !stamps || !step_sizes) return RELGNN_EINVAL;
  rows_adam_kernel<false, false><<<rows_grid(F), kBlock, 0, as_stream(stream)>>>(rowptr_t, nullptr, 0, F, p, nullptr, 0, m, v, ld, n / 4, stamps,
                                                                         const_cast<float*>(step_sizes), base, t_now, nullptr,
                                                                         0.f, 0.f, beta1, beta2, eps);
  return launch_status();
}

int relgnn_rows_adam_step(const int32_t* rowptr_t, int64_t F, float* p, const float* g, int64_t ld_g, float* m, float* v,
                          int64_t ld, int32_t n, int32_t* stamps, float* step_sizes, int32_t base, int32_t t_new,
                          const float* norm, float clip, float lr_t, float beta1, float beta2, float eps, void* stream) {
  if (F < 0 || F >= INT32_MAX || base < 0 || t_new <= base || !step_sizes || (clip > 0.f && !norm)) return RELGNN_EINVAL;
  if (!relgnn_rows_adam_supported(n)) return RELGNN_EUNSUPPORTED;
  if (F > 0 && (!rows_ok(p, ld, n) || !rows_ok(m, ld, n) || !rows_ok(v, ld, n) || !rows_ok(g, ld_g, n) || !stamps))
    return RELGNN_EINVAL;
  rows_adam_kernel<true, false><<<rows_grid(F), kBlock, 0, as_stream(stream)>>>(rowptr_t, nullptr, 0, F, p, g, ld_g, m, v, ld, n / 4, stamps,
                                                                        step_sizes, base, t_new, norm, clip, lr_t, beta1, beta2,
                                                                        eps);
  return launch_status();
}

int relgnn_rows_adam_step_compact(const int32_t* words, int64_t T, int64_t F, float* p, const float* g, int64_t ld_g, float* m,
                                  float* v, int64_t ld, int32_t n, int32_t* stamps, float* step_sizes, int32_t base, int32_t t_new,
                                  const float* norm, float clip, float lr_t, float beta1, float beta2, float eps, void* stream) {
  if (F < 0 || F >= INT32_MAX || T < 0 || T > F || base < 0 || t_new <= base || !step_sizes || (clip > 0.f && !norm))
    return RELGNN_EINVAL;
  if (!relgnn_rows_adam_supported(n)) return RELGNN_EUNSUPPORTED;
  if (T > 0 && (!words || !rows_ok(p, ld, n) || !rows_ok(m, ld, n) || !rows_ok(v, ld, n) || !rows_ok(g, ld_g, n) || !stamps))
    return RELGNN_EINVAL;
  // (T == 0: one block that stores the step size and finds no row)
  rows_adam_kernel<true, true><<<rows_grid(T), kBlock, 0, as_stream(stream)>>>(nullptr, words, F, T, p, g, ld_g, m, v, ld, n / 4,
                                                                              stamps, step_sizes, base, t_new, norm, clip, lr_t,
                                                                              beta1, beta2, eps);
  return launch_status();
}

}  // extern "C"
