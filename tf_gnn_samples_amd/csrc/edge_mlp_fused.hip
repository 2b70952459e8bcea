// The first per-edge product of an edge MLP with its left operand formed in flight (gnns/gnn_edge_mlp.py:95-102, gnns/rgin.py:114-119
// with >= 1 hidden layer; utils/utils.py:120-126 applied per edge type):
//
//     C[m, :] = out_act( in_act( P[row_src[m], :] + (Q ? Q[row_tgt[m], :] : 0) ) @ W_{type(m)} )          m in [0, M)
//
// P / Q are the node-side halves of the MLP's first Dense layer ([V*L, K] tables, rows node*L + type), in_act its activation: the
// [M, K] hidden tensor that relgnn_pair_materialize writes and the per-type products read back exists only as limb tiles in LDS here.
//
// Geometry, staging, k-tile order and the order of the six limb products are those of limb_gemm_sel_kernel (limb_gemm.hip): 128-row x
// 128-column panels, 8 waves = 2 row groups x 4 column tiles, three 24 KiB stages, waves 0-3 issue the DMA of the W limb blocks,
// waves 4-7 produce the left operand — thread x = tid & 255 owns row x & 127 and k-half x >> 7 of EVERY k-tile: its 32 bytes of the P
// row and of the Q row are loaded two k-tiles before they are added, activated (act_fwd_fast, the per-message activation behind
// act4_t of edge_fused.hip: the hidden values are bit for bit those of relgnn_pair_materialize) and split into the stage the barrier of
// the previous k-tile released.  A row's result therefore depends on its values and its weights alone, not on the panel it sits in:
// bit-identical to relgnn_pair_materialize followed by relgnn_limb_gemm_sel_xf32 per type block.
//
// What differs from that kernel:
//   panels   type blocks of the message list are no multiples of 128, so the panels come from a table {first message, rows (1..128),
//            weight index, 0} (graph.edge_mlp_panel_table): a panel never straddles an edge type; rows past its count are fed zeros
//            and not stored.  An entry that does not fit M / num_w is skipped.
//   in_act   a template argument (the activation sits between the loads and the split of every k-tile: a run-time switch there
//            would put seven inlined activations into the basic block of the MFMAs); out_act stays a run-time epilogue (act_rt).
//   rows     64-bit row addressing (M up to 2^31 - 1).
//   loads    issued by every wave outside any branch like there (see limb_gemm_kernel); a thread with nothing to produce re-reads
//            the first k-chunk of the panel's first message (always valid) instead of a zero block, and its values are zeroed.
// Resources (-Rpass-analysis=kernel-resource-usage, all 14 instantiations): 72 KiB of LDS, no scratch; without Q 111-114 VGPRs, with
// Q (a second 32-byte chunk in flight per register set) exactly 128 — two workgroups per CU either way.  With per-lane W block
// pointers the Q variants took 134-136 VGPRs and one workgroup per CU: 2324 instead of 2088 us on the C2 shape, slower than the
// composition (2301 us; profiles/edge_mlp_fused.jsonl).
#include "common.h"
#include "lds_dma.h"
#include "limb_frag.h"
#include "limb_split.h"

#include <type_traits>

using namespace relgnn;

namespace {

constexpr int BK = 16;
constexpr int EM_STAGES = 3;

struct EdgeMlpArgs {
  const float* P; int64_t ldp; const float* Q; int64_t ldq;
  const int32_t* row_src; const int32_t* row_tgt;
  const uint16_t* W; int64_t w_stride; int32_t num_w;
  const int32_t* panels; int32_t num_panels, chunks;
  float* C; int64_t ldc;
  int64_t M; int32_t N, K, out_act;
};

template <int IN_ACT, bool HASQ>
__global__ __launch_bounds__(512, 2) void edge_mlp_fwd_kernel(const EdgeMlpArgs a) {
  constexpr int TW = 2, T32 = 4, PR = 128, NC = 128;
  constexpr int PA = 3 * T32, PB = 3 * (NC / 32), NB = PA + PB;    // 12 + 12 blocks
  constexpr int STAGE_BYTES = NB * 1024;
  constexpr int G = PB / 4;
  __shared__ __attribute__((aligned(16))) unsigned char lds[EM_STAGES * STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int64_t lb = xcd_logical_block((int64_t)a.num_panels * a.chunks);
  if (lb < 0) return;
  const int q = (int)(lb / a.chunks), chunk = (int)(lb % a.chunks);
  const int4 pe = reinterpret_cast<const int4*>(a.panels)[q];
  const int64_t m0 = pe.x;
  const int rows_here = pe.y, wsel = pe.z;
  if (m0 < 0 || rows_here < 1 || rows_here > PR || m0 + rows_here > a.M || wsel < 0 || wsel >= a.num_w) return;   // (uniform)
  const int n0 = chunk * NC;
  const int ntiles = a.K / BK;
  const uint16_t* Wp = a.W + (int64_t)wsel * a.w_stride;

  // ---- W by DMA (waves 0-3) -------------------------------------------------------------------------------------------------
  const bool loader = wave < 4;
  constexpr int TILE = 3 * 512;
  // (wave-uniform block pointers + one per-lane offset: three per-lane 64-bit pointers would be six VGPRs, and the Q variants sit at
  //  the 128 that two workgroups per CU allow)
  const uint16_t* src[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int cb = (wave & 3) + 4 * g;
    src[g] = Wp + ((int64_t)(n0 / 32 + cb / 3) * ntiles) * TILE + (cb % 3) * 512;
  }
  const uint32_t lane_off = 8 * lane;
  auto issue_w = [&](int stage) {
    if (!loader) return;
    unsigned char* dst = lds + stage * STAGE_BYTES + PA * 1024;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      dma16(src[g] + lane_off, dst + ((wave & 3) + 4 * g) * 1024);
      src[g] += TILE;
    }
  };
  // (the loads of the left operand are issued by the loader waves too: a count that leaves them out waits for MORE of the older DMA
  //  instructions than necessary, never for fewer; counting them — vmcnt(G + 2 or 4) inside the k-loop — measured no different: 0.904
  //  against 0.907 of the composition's time on the C2 shape)
  auto wait_w = [&](int tiles) {
    if (!loader) return;
    if (tiles >= 1) wait_vm<G>(); else wait_vm<0>();
  };

  // ---- the left operand (waves 4-7): 32 B of the P row (+ 32 B of the Q row) per k-tile, two register sets (even / odd k-tiles),
  // each loaded two k-tiles before it is added, activated and split -------------------------------------------------------------
  const bool xwave = wave >= 4;
  const int x = tid & 255;
  const int xr = x & 127, xh_ = x >> 7;
  const bool xok = xwave && xr < rows_here;
  const int64_t xm = m0 + (xok ? xr : 0);              // (nothing to produce: the panel's first message, k-chunk 0)
  const float* pbase = a.P + (int64_t)a.row_src[xm] * a.ldp + (xok ? 8 * xh_ : 0);
  const float* qbase = nullptr;
  if constexpr (HASQ) qbase = a.Q + (int64_t)a.row_tgt[xm] * a.ldq + (xok ? 8 * xh_ : 0);
  const int xkmax = xok ? a.K - 16 : 0;
  const int xblock = (3 * (xr >> 5)) * 1024 + xh_ * 512 + (xr & 31) * 16;
  struct Chunk { f32x4 p[2]; f32x4 q[HASQ ? 2 : 1]; };
  Chunk xva, xvb;                                      // my chunk of an even / an odd k-tile in flight
  auto x_load = [&](Chunk& v, int kt) {                // (every wave, no branch; past the end: the last k-tile again)
    const int k = min(16 * kt, xkmax);
    v.p[0] = *reinterpret_cast<const f32x4*>(pbase + k);
    v.p[1] = *reinterpret_cast<const f32x4*>(pbase + k + 4);
    if constexpr (HASQ) {
      v.q[0] = *reinterpret_cast<const f32x4*>(qbase + k);
      v.q[1] = *reinterpret_cast<const f32x4*>(qbase + k + 4);
    }
  };
  auto x_split = [&](const Chunk& v, int kt) {         // my chunk of k-tile kt -> stage kt % 3
    float z[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float lo = v.p[0][i], hi = v.p[1][i];
      if constexpr (HASQ) { lo = lo + v.q[0][i]; hi = hi + v.q[1][i]; }
      z[i] = xok ? act_fwd_fast<IN_ACT>(lo) : 0.f;
      z[4 + i] = xok ? act_fwd_fast<IN_ACT>(hi) : 0.f;
    }
    uint4 h, m, l;
    split8(z, h, m, l);
    unsigned char* p = lds + (kt % EM_STAGES) * STAGE_BYTES + xblock;
    *reinterpret_cast<uint4*>(p) = h;
    *reinterpret_cast<uint4*>(p + 1024) = m;
    *reinterpret_cast<uint4*>(p + 2048) = l;
  };

  // ---- fragments / products -----------------------------------------------------------------------------------------------
  auto read_blk = [&](int stage, int blk) { return read_planes(lds + stage * STAGE_BYTES + blk * 1024 + 16 * lane, 1024); };
  f32x16 acc[TW];
#pragma unroll
  for (int tm = 0; tm < TW; ++tm)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tm][r] = 0.f;
  auto products = [&](f32x16 c, const Frag& w, const Frag& xx) { return limb_products(c, w, xx); };

  // ---- pipeline: k-tile t is multiplied while k-tile t+1 is complete in LDS and k-tile t+2 arrives (W by DMA, the left operand
  // from the register set of its parity, whose next load — k-tile t+4 — follows) ---------------------------------------------------
  issue_w(0);
  if (1 < ntiles) issue_w(1);
  x_load(xva, 0);
  x_load(xvb, 1);
  if (xwave) {
    x_split(xva, 0);
    if (1 < ntiles) x_split(xvb, 1);
  }
  x_load(xva, 2);
  x_load(xvb, 3);
  wait_w(min(1, ntiles - 1));
  wait_lgkm0();
  __builtin_amdgcn_s_barrier();
  Frag w_cur, w_nxt, x0, x1;
  w_cur = read_blk(0, PA + 3 * wn);
  x0 = read_blk(0, 3 * (wm * TW));
  auto ktile = [&](int t, auto odd_c) {
    constexpr int ODD = decltype(odd_c)::value;
    Chunk& xv = ODD ? xvb : xva;
    const int stage = t % EM_STAGES;
    const bool more = t + 1 < ntiles;
    if (t + 2 < ntiles) issue_w((t + 2) % EM_STAGES);
    if (xwave && t + 2 < ntiles) x_split(xv, t + 2);
    x_load(xv, t + 4);
    x1 = read_blk(stage, 3 * (wm * TW + 1));
    acc[0] = products(acc[0], w_cur, x0);
    if (more) {
      // W tile t+1 was issued at k-tile t-1 (or in the prologue); after it: W tile t+2 (this k-tile) and loads of the left operand
      wait_w(t + 2 < ntiles ? 1 : 0);
      wait_lgkm0();
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      w_nxt = read_blk((t + 1) % EM_STAGES, PA + 3 * wn);
      x0 = read_blk((t + 1) % EM_STAGES, 3 * (wm * TW));
    }
    acc[1] = products(acc[1], w_cur, x1);
    w_cur = w_nxt;
  };
  {
    int t = 0;
    for (; t + 1 < ntiles; t += 2) {
      ktile(t, std::integral_constant<int, 0>{});
      ktile(t + 1, std::integral_constant<int, 1>{});
    }
    if (t < ntiles) ktile(t, std::integral_constant<int, 0>{});
  }

  // ---- epilogue: a lane holds output row (lane & 31) x columns 8 c + 4 h + {0..3} of its 32 x 32 tiles -------------------------
  const int i32 = lane & 31, h32 = lane >> 5;
  const int colw = n0 + wn * 32;
#pragma unroll
  for (int tm = 0; tm < TW; ++tm) {
    const int r = (wm * TW + tm) * 32 + i32;
    if (r < rows_here) {
      float* crow = a.C + (m0 + r) * a.ldc;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = colw + 8 * c + 4 * h32;
        f32x4 v = f32x4{acc[tm][4 * c], acc[tm][4 * c + 1], acc[tm][4 * c + 2], acc[tm][4 * c + 3]};
        if (a.out_act != RELGNN_ACT_LINEAR) {
          v[0] = act_rt(a.out_act, v[0]); v[1] = act_rt(a.out_act, v[1]); v[2] = act_rt(a.out_act, v[2]); v[3] = act_rt(a.out_act, v[3]);
        }
        *reinterpret_cast<f32x4*>(crow + col) = v;
      }
    }
  }
}

inline bool act_id_ok(int32_t act) { return act >= RELGNN_ACT_LINEAR && act <= RELGNN_ACT_GELU; }

}  // namespace

extern "C" {

int relgnn_edge_mlp_fwd_supported(int32_t in_act, int32_t out_act, int32_t N, int32_t K) {
  return act_id_ok(in_act) && act_id_ok(out_act) && N > 0 && N % 128 == 0 && K % BK == 0 && K >= 16 && K <= 1024;
}

int relgnn_edge_mlp_fwd_xf32(int32_t in_act, int32_t out_act, const float* P, int64_t ldp, const float* Q, int64_t ldq,
                             const int32_t* row_src, const int32_t* row_tgt, const uint16_t* W_limbs, int32_t num_w,
                             const int32_t* panels, int32_t num_panels, float* C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                             void* stream) {
  if (M < 0 || M > INT32_MAX || N < 0 || K < 0 || num_w < 1 || num_panels < 0 || !act_id_ok(in_act) || !act_id_ok(out_act))
    return RELGNN_EINVAL;
  if (M == 0 || num_panels == 0) return RELGNN_OK;
  if (!P || !row_src || !W_limbs || !panels || !C || (Q && !row_tgt)) return RELGNN_EINVAL;
  if (!relgnn_edge_mlp_fwd_supported(in_act, out_act, N, K)) return RELGNN_EUNSUPPORTED;
  if (ldp % 4 || ldp < K || (Q && (ldq % 4 || ldq < K)) || ldc % 4 || ldc < N) return RELGNN_EUNSUPPORTED;
  if (!aligned16(P) || (Q && !aligned16(Q)) || !aligned16(W_limbs) || !aligned16(panels) || !aligned16(C)) return RELGNN_EUNSUPPORTED;
  EdgeMlpArgs a{};
  a.P = P; a.ldp = ldp; a.Q = Q; a.ldq = ldq; a.row_src = row_src; a.row_tgt = row_tgt;
  a.W = W_limbs; a.w_stride = relgnn_limb_elements(N, K); a.num_w = num_w;
  a.panels = panels; a.num_panels = num_panels; a.chunks = N / 128;
  a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.out_act = out_act;
  const int64_t logical = (int64_t)num_panels * a.chunks;
  const unsigned grid = (unsigned)(8 * ((logical + 7) / 8));
  hipStream_t st = as_stream(stream);
  RELGNN_DISPATCH_ACT(in_act, ACT, {
    if (Q) edge_mlp_fwd_kernel<ACT, true><<<grid, 512, 0, st>>>(a);
    else edge_mlp_fwd_kernel<ACT, false><<<grid, 512, 0, st>>>(a);
  });
  return launch_status();
}

}  // extern "C"
