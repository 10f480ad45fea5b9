// Split fp16 LDS images of fp32 operand tiles whose MFMA reduction runs over ROWS (weight gradients Wbar = Y^T X): shared by
// k_gemm_tn_tr (pp_gemm_tn_tr.h, scene branch) and k_wgrad_chain_s (pp_mlp_split.hip, object branch).
// An image is [64 rows][128 halfs] with 256-byte rows whose 16-byte chunks are XOR-swizzled (cdna_hip_programming.md T10, image
// (b)).  A thread stores what it loaded - four consecutive columns of a row, scaled and split into hi | lo, as two conflict-free
// 8-byte stores - and a wavefront reads an MFMA fragment (eight consecutive rows of one column per lane) as two hardware-transposed
// reads (ds_read_b64_tr_b16) of 4 rows x 16 columns per 16-lane group.  The transposed reads need EXEC all ones: call tn_frag
// from wave-uniform control flow only.
#pragma once
#include "pp_gemm_split.h"

// byte offset of 16-byte chunk `ch` (0..15) of row `row`
__device__ __forceinline__ int tn_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// columns 4 c4 .. 4 c4 + 3 of row `row`: x * s split into the hi and lo images
__device__ __forceinline__ void tn_store4(unsigned char* hi, unsigned char* lo, int row, int c4, float4 x, float s) {
  const int o = tn_off(row, c4 >> 1) + 8 * (c4 & 1);
  pp_half4 h, l;
  pp_split4(x, s, h, l);
  *reinterpret_cast<pp_half4*>(hi + o) = h;
  *reinterpret_cast<pp_half4*>(lo + o) = l;
}

// MFMA fragment of columns cb .. cb + 31, rows ks .. ks + 15: lane l receives column cb + (l & 31), rows ks + 8 (l >> 5) .. + 7.
// Lane (group g = lane / 16, q = (lane & 15) / 4, p = lane & 3) addresses row q, columns 4 p .. 4 p + 3 of its group's 4 x 16
// block and receives column (lane & 15) of the block's four rows; two blocks = the eight rows of the lane's half.
__device__ __forceinline__ pp_half8 tn_frag(const unsigned char* plane, int cb, int ks, int lane) {
  typedef __fp16 tn_h4 __attribute__((vector_size(8)));
  typedef __fp16 tn_h8 __attribute__((vector_size(16)));
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fp = lane & 3;
  const int ch = ((cb + 16 * (fg & 1)) >> 3) + (fp >> 1);
  const int row = ks + 8 * (fg >> 1) + fq;
  const tn_h4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) tn_h4*)(plane + tn_off(row, ch) + 8 * (fp & 1)));
  const tn_h4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) tn_h4*)(plane + tn_off(row + 4, ch) + 8 * (fp & 1)));
  const tn_h8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(pp_half8, v);
}
