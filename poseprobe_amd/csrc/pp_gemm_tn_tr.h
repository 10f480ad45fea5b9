// Split-precision weight gradient of the scene branch (pp_nerf.hip is its only user):  Wbar[n][k] += sum_r Y[r][n] X[r][k]
// (one 128 x 128 block per blockIdx.y, row splits along blockIdx.x, as k_gemm_tn), three fp16 products per fp32 product with
// the scales of pp_gemm_split.h.  The reduction runs over ROWS, so an MFMA operand fragment is 8 consecutive rows of one column.
// Row-major LDS images and hardware-transposed fragment reads (pp_split_image.h).  The first generation transposed on
// the way INTO LDS: 16-byte stores of eight rows of one column, 4-way bank conflicts by construction - on the LDS store path
// (13 cycles per conflict-free ds_write_b128 already, MI355X_MICROARCH.md LDS table) that was ~32 cycles per wave-instruction,
// 64 of them per chunk and work-group: more LDS time than the chunk's matrix instructions (PMC: matrix pipe busy 25 %).  Here a
// thread stores what it loaded - four consecutive columns of a row, hi and lo, as 8-byte conflict-free stores - and a
// fragment is two transposed reads.
#pragma once
#include "pp_ordered.h"
#include "pp_split_image.h"

// slot of a work-group in the ordered-flush workspace (floats): the 128 x 128 block in accumulator order | 128 bias sums
#define TN_ORD_SLOT ORD_WGRAD_SLOT
#define TN_ORD_BIAS ORD_WGRAD_BIAS

static __global__ __launch_bounds__(256, 2) void k_gemm_tn_tr(const float* __restrict__ Y_, int ldy, const float* __restrict__ X_, int ldx,
                                                          int Kx_, float* __restrict__ Wbar_, int ldwb, float* __restrict__ bbar_,
                                                          const int32_t* __restrict__ count, int rcap,
                                                          const float* __restrict__ y_max, const float* __restrict__ x_max,
                                                          float* __restrict__ ord) {
  constexpr int CH = 64;
  __shared__ __attribute__((aligned(1024))) unsigned char img[4 * CH * 256];       // Yh | Yl | Xh | Xl
  unsigned char* const Yh = img;
  unsigned char* const Yl = img + CH * 256;
  unsigned char* const Xh = img + 2 * CH * 256;
  unsigned char* const Xl = img + 3 * CH * 256;
  const int nkb = (Kx_ + 127) >> 7;
  const int nb = blockIdx.y / nkb, kb = blockIdx.y - nb * nkb;
  const float* __restrict__ Y = Y_ + nb * 128;
  const float* __restrict__ X = X_ + kb * 128;
  const int Kx = min(128, Kx_ - kb * 128);
  float* __restrict__ Wbar = Wbar_ + (size_t)nb * 128 * ldwb + kb * 128;
  float* __restrict__ bbar = (bbar_ && kb == 0) ? bbar_ + nb * 128 : nullptr;
  const int R = min(count[0], rcap);
  const int rows_per_wg = ((R + (int)gridDim.x - 1) / (int)gridDim.x + CH - 1) / CH * CH;
  const int rb = blockIdx.x * rows_per_wg;
  if (rb >= R) return;
  const int re = min(rb + rows_per_wg, R);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const float sY = pp_split_scale(y_max[0]), sX = pp_split_scale(x_max[0]);
  const int c4 = tid & 31, rblk = tid >> 5;                 // this thread: columns 4 c4 .. 4 c4 + 3, rows 8 rblk .. 8 rblk + 7
  const int kx4 = Kx >> 2;
  f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][u][i] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  // rows i0 .. i1 - 1 of this thread's eight of the chunk at r0: clamped addresses, no branches (rows past the range and columns
  // past Kx are zeroed when they are converted) - the fetches of the next chunk are issued in FOUR pieces between the matrix
  // instructions of this one.  All sixteen in front of them cost 2 k ticks per chunk (phase timers with the fetches removed:
  // matrix phase 4.5 k -> 2.5 k): 8 wavefronts x 16 KB pass the CU's 64 B / clock address-and-data path in ~2 k cycles, and a
  // wavefront's matrix instructions cannot issue before the fetches in front of them have
  float4 ry[8], rx[8];
  auto load_rows = [&](int r0, int i0, int i1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < i0 || i >= i1) continue;
      const int gr = min(r0 + rblk * 8 + i, R - 1);
      ry[i] = *reinterpret_cast<const float4*>(Y + (size_t)gr * ldy + c4 * 4);
      rx[i] = *reinterpret_cast<const float4*>(X + (size_t)gr * ldx + (c4 < kx4 ? c4 : 0) * 4);
    }
  };
  auto frag = [&](const unsigned char* plane, int cb, int ks) { return tn_frag(plane, cb, ks, lane); };
  load_rows(rb, 0, 8);
  for (int r0 = rb; r0 < re; r0 += CH) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float ky = (r0 + rblk * 8 + i < re) ? 1.f : 0.f, kx = (c4 < kx4) ? ky : 0.f;
      ry[i].x *= ky; ry[i].y *= ky; ry[i].z *= ky; ry[i].w *= ky;
      rx[i].x *= kx; rx[i].y *= kx; rx[i].z *= kx; rx[i].w *= kx;
      tn_store4(Yh, Yl, rblk * 8 + i, c4, ry[i], sY);
      tn_store4(Xh, Xl, rblk * 8 + i, c4, rx[i], sX);
    }
    if (bbar) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { bsum[0] += ry[i].x; bsum[1] += ry[i].y; bsum[2] += ry[i].z; bsum[3] += ry[i].w; }
    }
    __syncthreads();
    if (wc * 64 < Kx) {                                       // (uniform per wavefront: the transposed reads need all 64 lanes)
      // fragments of the next 16 rows are on their way while the matrix instructions of these 16 issue (left in one loop
      // body, the compiler reads a step's ten fragments only after the previous step's last matrix instruction: four exposed
      // LDS round trips per chunk - phase timers: 4.4 k ticks per chunk of 48 matrix instructions)
      pp_half8 fa[2][4], fb[2][4];                          // [parity][tile 0 hi, tile 0 lo, tile 1 hi, tile 1 lo]
      auto fetch = [&](int par, int ks) {
#pragma unroll
        for (int t = 0; t < 2; ++t) { fa[par][2 * t] = frag(Yh, wr * 64 + t * 32, ks); fa[par][2 * t + 1] = frag(Yl, wr * 64 + t * 32, ks); }
#pragma unroll
        for (int u = 0; u < 2; ++u) { fb[par][2 * u] = frag(Xh, wc * 64 + u * 32, ks); fb[par][2 * u + 1] = frag(Xl, wc * 64 + u * 32, ks); }
      };
      fetch(0, 0);
#pragma unroll
      for (int s4 = 0; s4 < CH / 16; ++s4) {
        const int par = s4 & 1;
        if (s4 + 1 < CH / 16) fetch(par ^ 1, (s4 + 1) * 16);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[par][2 * t + 1], fb[par][2 * u], acc[t][u], 0, 0, 0);
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[par][2 * t], fb[par][2 * u + 1], acc[t][u], 0, 0, 0);
            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[par][2 * t], fb[par][2 * u], acc[t][u], 0, 0, 0);
          }
          if (t == 0) {                    // a quarter of the next chunk's rows behind the first six matrix instructions
            __builtin_amdgcn_sched_barrier(0);
            load_rows(r0 + CH, 2 * s4, 2 * s4 + 2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    } else {
      load_rows(r0 + CH, 0, 8);                               // a wavefront without columns in this block still stages its rows
    }
    __syncthreads();
  }
  const float inv = 1.0f / (sY * sX);
  // ordered flush (ord != nullptr, uniform over the launch): the scaled block as it lies in the registers and the bias sums go
  // into slot (blockIdx.y, blockIdx.x) with plain stores, k_gemm_tn_tr_reduce adds the slots of a block in a fixed order
  float* __restrict__ slot = ord ? ord + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * TN_ORD_SLOT : nullptr;
  if (slot) {
    if (wc * 64 < Kx) {
      float4* __restrict__ s4 = reinterpret_cast<float4*>(slot);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            s4[((t * 2 + u) * 4 + q) * 256 + tid] = make_float4(acc[t][u][4 * q] * inv, acc[t][u][4 * q + 1] * inv,
                                                                acc[t][u][4 * q + 2] * inv, acc[t][u][4 * q + 3] * inv);
    }
  } else if (wc * 64 < Kx) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int k = wc * 64 + u * 32 + l31;
        if (k >= Kx) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int n = wr * 64 + t * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
          atomicAdd(&Wbar[(size_t)n * ldwb + k], acc[t][u][reg] * inv);
        }
      }
  }
  if (bbar) {                              // 8 row blocks x 128 columns of partial sums -> one atomic per column
    float* red = reinterpret_cast<float*>(img);           // the operand images are dead (last chunk ended with a barrier)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[rblk * 128 + c4 * 4 + j] = bsum[j];
    __syncthreads();
    if (tid < 128) {
      float sum = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) sum += red[q * 128 + tid];
      if (slot) slot[TN_ORD_BIAS + tid] = sum;
      else atomicAdd(&bbar[tid], sum);
    }
  }
}

// Behind k_gemm_tn_tr with `ord` on the same stream (grid: TN_ORD_SLOT / 256 x the product's output blocks, ORD_RED_THREADS):
// Wbar / bbar += the sum over the ACTIVE row splits of an output block's slots, splits added in the order of pp_ordered_rows_sum,
// one writer per address.  The active count is derived from `count` with the producer's own expression (its work-groups with
// rb >= R return before the flush): an idle slot is never read, nor is an entry its producer did not write (columns past Kx,
// bias sums of a block that carries none).
static __global__ __launch_bounds__(ORD_RED_THREADS) void k_gemm_tn_tr_reduce(const float* __restrict__ ord, int splits, int Kx_,
                                                                              float* __restrict__ Wbar_, int ldwb,
                                                                              float* __restrict__ bbar_,
                                                                              const int32_t* __restrict__ count, int rcap) {
  __shared__ float4 lds[ORD_RED_GROUPS * 64];
  constexpr int CH = 64;
  const int nkb = (Kx_ + 127) >> 7;
  const int nb = blockIdx.y / nkb, kb = blockIdx.y - nb * nkb;
  const int Kx = min(128, Kx_ - kb * 128);
  const int R = min(count[0], rcap);
  if (R <= 0) return;
  const int rows_per_wg = ((R + splits - 1) / splits + CH - 1) / CH * CH;
  const int active = (R + rows_per_wg - 1) / rows_per_wg;          // the work-groups with blockIdx.x * rows_per_wg < R
  const int e4 = blockIdx.x * 64 + (threadIdx.x & 63);
  // entry e4 of a slot: (tile t, u | register group q | thread tid) of the accumulator block, then 32 float4s of bias sums
  const int tid = e4 & 255, q = (e4 >> 8) & 3, u = (e4 >> 10) & 1, t = (e4 >> 11) & 1;
  const int lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int k = wc * 64 + u * 32 + (lane & 31);
  const bool is_bias = e4 >= TN_ORD_BIAS / 4;
  const bool valid = is_bias ? (e4 < TN_ORD_SLOT / 4 && bbar_ && kb == 0) : (k < Kx);
  float4 s;
  if (!pp_ordered_rows_sum(reinterpret_cast<const float4*>(ord), TN_ORD_SLOT / 4, blockIdx.y * splits, active, e4, valid, lds, s)) return;
  if (is_bias) {
    float* __restrict__ b = bbar_ + nb * 128 + 4 * (e4 - TN_ORD_BIAS / 4);      // (a bias block need not be 16-byte aligned)
    b[0] += s.x; b[1] += s.y; b[2] += s.z; b[3] += s.w;
    return;
  }
  float* __restrict__ W = Wbar_ + (size_t)nb * 128 * ldwb + kb * 128 + k;
  const int n = wr * 64 + t * 32 + 8 * q + 4 * (lane >> 5);
  W[(size_t)n * ldwb] += s.x;
  W[(size_t)(n + 1) * ldwb] += s.y;
  W[(size_t)(n + 2) * ldwb] += s.z;
  W[(size_t)(n + 3) * ldwb] += s.w;
}
