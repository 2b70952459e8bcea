// Hand-over between wave roles of one workgroup through monotonic counters in LDS (rgcn_fused.hip, limb_gemm_pc.hip,
// limb_gemm_pc_typed.hip, gru_cell.hip forward and backward): the pieces these kernels share.  gfx950 only.
#pragma once
#include "common.h"
#include "lds_dma.h"

namespace relgnn {

constexpr int HANDOVER_SPIN_LIMIT = 1 << 22;     // a poll that takes this long is a bug: give up, flag it, finish with wrong numbers

// a relaxed workgroup-scope atomic load: ds_read_b32 (a volatile load becomes a flat load behind vmcnt(0) lgkmcnt(0))
__device__ __forceinline__ int handover_counter(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void handover_fence() { asm volatile("" ::: "memory"); }

// The caller's status block (device memory, int32[2], may be null = nothing is reported; include/relgnn.h RELGNN_HANDOVER_*):
//   [0]  give-up bits, OR-ed in by a kernel whose poll ran out: RELGNN_HANDOVER_FUSED_MATRIX / _FUSED_GATHER a matrix / gather wave
//        of rgcn_fused_kernel; RELGNN_HANDOVER_PC_MATRIX / _PC_PRODUCER a matrix / producer wave of limb_gemm_pc_kernel,
//        limb_gemm_pct_kernel, gru_cell_fwd_kernel or gru_cell_bwd_kernel.  The caller zeroes it and reads it where it syncs anyway.
//   [1]  the poll bound, 0 = HANDOVER_SPIN_LIMIT (tests write 1 to make every poll give up at once).
__device__ __forceinline__ int handover_limit(const int32_t* status) {
  const int v = status ? __builtin_amdgcn_readfirstlane(status[1]) : 0;
  return v > 0 ? v : HANDOVER_SPIN_LIMIT;
}

// Wait until *counter >= target, for at most `limit` rounds.  A poll that runs out sets the wave's `dead` flag — it stops waiting
// for anything from then on — and ORs `give_up_bit` (RELGNN_HANDOVER_*) into status[0].  Returns the rounds it waited (what the
// timing builds count).  (`limit` and `status` by reference and the caller's own `lane`, as the kernels' poll lambdas captured
// them: by value, or with the lane taken from threadIdx here, hipcc places the scalar code around the polls differently — other
// SGPRs, scalar instructions in other slots — and this header is meant to change no instruction of its users.  Observed with
// hipcc of ROCm 7.2.0, AMD clang 22.0.0git; profiles/kernel_helpers.txt.)
__device__ __forceinline__ int handover_poll(int* counter, int target, const int& limit, bool& dead, int32_t* const& status,
                                             int give_up_bit, int lane) {
  if (dead) return 0;
  int spins = 0;
  while (__builtin_amdgcn_readfirstlane(handover_counter(counter)) < target) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > limit) { dead = true; if (lane == 0 && status) atomicOr(status, give_up_bit); break; }
  }
  handover_fence();
  return spins;
}

// *counter += by, behind the LDS accesses of this wave that the count reports
__device__ __forceinline__ void handover_signal(int* counter, int by) {
  wait_lgkm0();
  handover_fence();
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(counter, by, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace relgnn
