// Ray-level terms of object_losses (lib/losses.py:26-29, :42-45, :66): the per-ray expressions and the batch's masked-pixel count,
// shared by k_loss_rays (pp_loss.hip, one thread per ray) and k_march_loss_bwd (pp_march.hip, one wavefront per ray).
#pragma once
#include "pp_common.h"

__device__ __forceinline__ float block_sum256(float v, float* sm) {
  v = pp_wave_sum(v);
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wid] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// number of masked-in pixels of the batch: every block (256 threads) sums the (few KB of) masks itself, in k_sum's order, instead
// of waiting for a separate single-block kernel
__device__ __forceinline__ float loss_mask_sum(const float* __restrict__ mask_px, int n_rays, float* sm) {
  float part = 0.f;
  for (int i = threadIdx.x; i < n_rays; i += 256) part += mask_px[i];
  return block_sum256(part, sm);
}

struct RayLoss { float g_rgbm[3], g_last, g_cw, l_mse, l_ent, l_bce; };

// one ray: rgbm = clamped composited colour, a = alphainv_last, c0 = cum_weights, y = its mask pixel
__device__ __forceinline__ RayLoss loss_ray_terms(const float (&rgbm)[3], const float a, const float c0, const float (&target)[3],
                                                  const float y, const float msum, const float invN, const float w_main,
                                                  const float w_ent, const float w_mask, const float ls) {
  RayLoss L;
  L.l_mse = 0.f;
  for (int k = 0; k < 3; ++k) {
    float d = rgbm[k] * y - target[k] * y;
    L.l_mse += d * d;
    L.g_rgbm[k] = ls * w_main * 2.f * d * y / (msum * 3.f);
  }
  float p = fminf(fmaxf(a, 1e-6f), 1.f - 1e-6f);
  float lp = logf(p), lq = logf(1.f - p);
  L.l_ent = -(p * lp + (1.f - p) * lq);
  L.g_last = (a >= 1e-6f && a <= 1.f - 1e-6f) ? ls * w_ent * (-(lp - lq)) * invN : 0.f;
  float c = fminf(fmaxf(c0, 1e-3f), 1.f - 1e-3f);
  L.l_bce = -(y * logf(c) + (1.f - y) * logf(1.f - c));
  L.g_cw = (c0 >= 1e-3f && c0 <= 1.f - 1e-3f) ? ls * w_mask * (-(y / c) + (1.f - y) / (1.f - c)) * invN : 0.f;
  return L;
}

// sums of the three terms over some rays -> loss_out (atomic +=)
__device__ __forceinline__ void loss_rays_add(float* __restrict__ loss_out, const float l_mse, const float l_ent, const float l_bce,
                                              const float msum, const float invN, const float w_main, const float w_ent,
                                              const float w_mask) {
  atomicAdd(&loss_out[0], l_mse / (msum * 3.f));
  atomicAdd(&loss_out[1], l_ent * invN);
  atomicAdd(&loss_out[6], l_bce * invN);
  // [7]: the WEIGHTED sum of all terms (both kernels add their share): object_losses' `loss` without the TV term
  atomicAdd(&loss_out[7], w_main * (l_mse / (msum * 3.f)) + w_ent * (l_ent * invN) + w_mask * (l_bce * invN));
}
