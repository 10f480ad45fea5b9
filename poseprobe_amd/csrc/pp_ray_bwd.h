// Ray / pose backward bodies shared by their stand-alone kernels (pp_rays.hip) and by the optimiser launch that carries them as
// work-group roles beside the grid pass (pp_optim.hip, k_grid_tv_adam_tail).
#pragma once
#include "pp_common.h"
#include "pp_ordered.h"

// torch's CPU norm kernel accumulates with fused multiply-adds: sqrt(fma(z,z,fma(y,y,x*x))) (probed)
__device__ __forceinline__ float pp_norm3(float x, float y, float z) {
  return sqrtf(fmaf(z, z, fmaf(y, y, pp_mul(x, x))));
}

__device__ __forceinline__ void pixel_dir(int idx, int H, int W, const float* __restrict__ intr, int inverse_y,
                                          int& view, float dirs[3]) {
  view = idx / (H * W);
  int rem = idx - view * (H * W);
  int pj = rem / W, pi = rem - pj * W;
  float fi = pp_add((float)pi, 0.5f), fj = pp_add((float)pj, 0.5f);
  const float* K = intr + view * 4;
  dirs[0] = pp_div(pp_sub(fi, K[2]), K[0]);
  float y = pp_div(pp_sub(fj, K[3]), K[1]);
  dirs[1] = inverse_y ? y : -y;
  dirs[2] = inverse_y ? 1.f : -1.f;
}

// one element (view, k) of se3_grad = jac^T c2w_grad.  ARRIVED: c2w_grad was summed by other work-groups of THIS launch - its
// words are read by agent-scope atomic loads (served where the atomics were performed, never by this compute unit's L1)
template <bool ARRIVED>
__device__ __forceinline__ float pose_bwd_elem(const float* __restrict__ jac, const float* c2w_grad, int t) {
  int v = t / 6, k = t % 6;
  float s = 0.f;
  for (int e = 0; e < 12; ++e) {
    const float g = ARRIVED ? __hip_atomic_load(c2w_grad + v * 12 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : c2w_grad[v * 12 + e];
    s += jac[(v * 12 + e) * 6 + k] * g;
  }
  return s;
}

// ------------------------------------------------------------------------------------------------
// backward: samples -> rays -> c2w.  One wavefront per ray; work-group `block` of 256 threads owns rays 4 * block ...
// s_c2w: [n_views*12] floats of LDS.  RETURNING: the work-group's sums are added to c2w_grad by RETURNING atomics and every
// wavefront waits for its ones - when the function returns, the additions have been performed (the caller may count an arrival).
// ------------------------------------------------------------------------------------------------
template <bool RETURNING>
__device__ __forceinline__ void raygen_bwd_body(
    int block, float* s_c2w, const SceneDev& sc, const int32_t* __restrict__ ray_idx, int n_rays, const float* __restrict__ c2w,
    const float* __restrict__ intr, int n_views, int H, int W, int inverse_y, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ t_min, const int32_t* __restrict__ ray_start,
    const float* __restrict__ pts_grad, const float* __restrict__ step, const float* __restrict__ vgrad_s,
    const float* __restrict__ g_o_in, const float* __restrict__ g_d_in, const float* __restrict__ g_v_in,
    const float* __restrict__ g_depth, float* __restrict__ g_o_out, float* __restrict__ g_d_out,
    float* __restrict__ g_v_out, float* __restrict__ c2w_grad, float* __restrict__ part) {
  for (int i = threadIdx.x; i < n_views * 12; i += blockDim.x) s_c2w[i] = 0.f;
  __syncthreads();
  int r = block * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r < n_rays) {
    int b = ray_start[r], e = ray_start[r + 1];
    float s0[3] = {0, 0, 0}, s1[3] = {0, 0, 0}, gv[3] = {0, 0, 0};
    for (int i = b + lane; i < e; i += 64) {
      float st = step[i];
      for (int k = 0; k < 3; ++k) {
        float g = pts_grad[i * 3 + k];
        s0[k] += g;
        s1[k] += g * st;
        if (vgrad_s) gv[k] += vgrad_s[i * 3 + k];
      }
    }
    for (int k = 0; k < 3; ++k) { s0[k] = pp_wave_sum(s0[k]); s1[k] = pp_wave_sum(s1[k]); gv[k] = pp_wave_sum(gv[k]); }
    if (lane == 0) {
      float o[3], d[3];
      for (int k = 0; k < 3; ++k) { o[k] = rays_o[r * 3 + k]; d[k] = rays_d[r * 3 + k]; }
      float nrm = pp_norm3(d[0], d[1], d[2]);
      float tm = t_min[r];
      float gdep = g_depth ? g_depth[r] : 0.f;
      float ob[3], db[3];
      float tmin_bar = gdep / nrm, nrm_bar = -gdep * tm / (nrm * nrm);
      float s1d = 0.f;
      for (int k = 0; k < 3; ++k) {
        ob[k] = s0[k];
        db[k] = s0[k] * tm + s1[k] / nrm;
        tmin_bar += s0[k] * d[k];
        s1d += s1[k] * d[k];
      }
      nrm_bar -= s1d / (nrm * nrm);
      for (int k = 0; k < 3; ++k) db[k] += nrm_bar * d[k] / nrm;
      // slab test backward (amax / minimum / clamp with torch's tie handling)
      float ra[3], rb[3], lo[3], vec[3];
      float tm_raw = -INFINITY;
      for (int k = 0; k < 3; ++k) {
        vec[k] = (d[k] == 0.f) ? 1e-6f : d[k];
        ra[k] = (sc.mx[k] - o[k]) / vec[k];
        rb[k] = (sc.mn[k] - o[k]) / vec[k];
        lo[k] = fminf(ra[k], rb[k]);
        tm_raw = fmaxf(tm_raw, lo[k]);
      }
      if (tm_raw >= sc.near_ && tm_raw <= sc.far_ && tmin_bar != 0.f) {
        int nmax = 0;
        for (int k = 0; k < 3; ++k) nmax += (lo[k] == tm_raw);
        for (int k = 0; k < 3; ++k) {
          if (lo[k] != tm_raw) continue;
          float lb = tmin_bar / (float)nmax;
          float wa = ra[k] < rb[k] ? 1.f : (ra[k] == rb[k] ? 0.5f : 0.f);
          float rab = lb * wa, rbb = lb * (1.f - wa);
          ob[k] -= (rab + rbb) / vec[k];
          if (d[k] != 0.f) db[k] -= (rab * ra[k] + rbb * rb[k]) / vec[k];
        }
      }
      if (g_o_in) for (int k = 0; k < 3; ++k) ob[k] += g_o_in[r * 3 + k];
      if (g_d_in) for (int k = 0; k < 3; ++k) db[k] += g_d_in[r * 3 + k];
      if (g_v_in) for (int k = 0; k < 3; ++k) gv[k] += g_v_in[r * 3 + k];
      if (g_o_out) for (int k = 0; k < 3; ++k) g_o_out[r * 3 + k] = ob[k];
      if (g_d_out) for (int k = 0; k < 3; ++k) g_d_out[r * 3 + k] = db[k];
      if (g_v_out) for (int k = 0; k < 3; ++k) g_v_out[r * 3 + k] = gv[k];
      if (c2w_grad) {
        // Voxurf variant: rays_d = viewdirs = normalize(R dirs) -> one tensor (voxurf_coarse.py:1404)
        int view;
        float dirs[3];
        pixel_dir(ray_idx[r], H, W, intr, inverse_y, view, dirs);
        const float* P = c2w + view * 12;
        float Du[3], gt[3];
        for (int k = 0; k < 3; ++k) {
          Du[k] = dirs[0] * P[k * 4 + 0] + dirs[1] * P[k * 4 + 1] + dirs[2] * P[k * 4 + 2];
          gt[k] = db[k] + gv[k];
        }
        float Dn = sqrtf(Du[0] * Du[0] + Du[1] * Du[1] + Du[2] * Du[2]);
        float nh[3] = {Du[0] / Dn, Du[1] / Dn, Du[2] / Dn};
        float dot = nh[0] * gt[0] + nh[1] * gt[1] + nh[2] * gt[2];
        // part != nullptr (ordered flush, pp_ordered.h): the ray's twelve contributions and its view go to the ray's row,
        // k_raygen_c2w_reduce adds the rows of a view in ray order
        float* __restrict__ row = part ? part + (size_t)r * ORD_RAY_ROW : nullptr;
        for (int k = 0; k < 3; ++k) {
          float Db = (gt[k] - nh[k] * dot) / Dn;
          if (row) {
            for (int j = 0; j < 3; ++j) row[k * 4 + j] = Db * dirs[j];
            row[k * 4 + 3] = ob[k];
          } else {
            for (int j = 0; j < 3; ++j) atomicAdd(&s_c2w[view * 12 + k * 4 + j], Db * dirs[j]);
            atomicAdd(&s_c2w[view * 12 + k * 4 + 3], ob[k]);
          }
        }
        if (row) row[12] = __int_as_float(view);
      }
    }
  }
  __syncthreads();
  if (c2w_grad && !part)
    for (int i = threadIdx.x; i < n_views * 12; i += blockDim.x)
      if (s_c2w[i] != 0.f) {
        if (RETURNING) {
          float old = __hip_atomic_fetch_add(&c2w_grad[i], s_c2w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          asm volatile("" ::"v"(old));               // the returned value is "used": the returning form stays
        } else {
          atomicAdd(&c2w_grad[i], s_c2w[i]);
        }
      }
  if (RETURNING) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
