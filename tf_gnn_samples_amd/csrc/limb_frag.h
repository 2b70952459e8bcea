// What every exact-split kernel shares on the matrix-pipe side: the vector types, the limb fragment of one MFMA operand, its read
// from three planes, THE order of the limb products of a k-tile, and the sub-slab geometry of the wave-role kernels.  gfx950 only.
#pragma once
#include "common.h"

namespace relgnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// one lane's share of a 32 x 16 operand tile (row lane & 31, k = 8 (lane >> 5) .. + 7) as limbs: three bf16 planes, or two fp16
// planes (hi, lo) carried in the same registers
struct Frag { bf16x8 hi, mid, lo; };

// the planes of a fragment lie `plane_stride` bytes apart (NL = 2: hi, lo; `mid` is a copy that nobody multiplies)
template <int NL = 3>
__device__ __forceinline__ Frag read_planes(const unsigned char* p, int plane_stride) {
  Frag f;
  f.hi = *reinterpret_cast<const bf16x8*>(p);
  if constexpr (NL == 3) {
    f.mid = *reinterpret_cast<const bf16x8*>(p + plane_stride);
    f.lo = *reinterpret_cast<const bf16x8*>(p + 2 * plane_stride);
  } else {
    f.lo = *reinterpret_cast<const bf16x8*>(p + plane_stride);
    f.mid = f.lo;
  }
  return f;
}

// acc += w * x over one k-tile, from the limbs.  The order is the package's bit-identity contract: every kernel that claims the
// bits of another accumulates a k-tile's products in THIS order — small terms first: the three 2^-16 products, then the two 2^-8
// ones, then the leading one (NL = 2, two fp16 limbs behind power-of-two scales: hi lo, lo hi, hi hi).
template <int NL = 3>
__device__ __forceinline__ f32x16 limb_products(f32x16 acc, const Frag& w, const Frag& x) {
  if constexpr (NL == 2) {
    const f16x8 wh = __builtin_bit_cast(f16x8, w.hi), wl = __builtin_bit_cast(f16x8, w.lo);
    const f16x8 xh = __builtin_bit_cast(f16x8, x.hi), xl = __builtin_bit_cast(f16x8, x.lo);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.hi, x.lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.lo, x.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.mid, x.mid, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.hi, x.mid, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.mid, x.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.hi, x.hi, acc, 0, 0, 0);
  }
  return acc;
}

// A sub-slab — what the producer waves of a wave-role kernel hand to its matrix waves: one 32-row tile x PIECES * 8 k as limbs.
// A piece is 32 rows x 16 B (8 k of one limb) + 16 B, so that consecutive pieces start in consecutive bank quads; a plane is the
// PIECES (k-tile, k half) pieces of one limb; a slab is the three planes.  PIECES = 16: 32 rows x 128 k, 25 344 B (limb_gemm_pc.hip,
// limb_gemm_pc_typed.hip, gru_cell.hip); 32: 32 rows x 256 k, 50 688 B (rgcn_fused.hip: a whole gathered row).
template <int PIECES>
struct SubSlab {
  static constexpr int PIECE = 528, PLANE = PIECES * PIECE, SLAB = 3 * PLANE;
};

}  // namespace relgnn
