// SPARF correspondence loss of the scene branch on depths rendered by the scene pass, and the fold of the matched rows' ray
// gradients into the pose gradient.
//
//   reference: lib/bg_nerf/source/training/core/corres_loss.py
//     :93-138   compute_render_and_repro_loss_w_repro_thres   (one direction: re-project, optional filters, Huber)
//     :140-222  compute_loss_pairwise                          (both directions, coarse + fine, / 2 or / 4)
//   lib/bg_nerf/source/utils/geometry/batched_geometry_utils.py:199-228 (project_to_other_img),
//   lib/bg_nerf/source/training/core/base_losses.py:197-224 (compute_diff_loss), utils/camera.py:37-66 (pose_inverse_4x4).
//
// Both kernels are one work-group with a fixed summation order (strided per-thread partials, then a tree over the 256
// partials), no atomics: the same inputs give the same bits, as k_nerf_huber.
#include "pp_common.h"

#define CORR_T 256

// huber_loss(x, 0, delta = 1) and its derivative (torch: |x| < delta ? 0.5 x^2 : delta (|x| - 0.5 delta))
__device__ __forceinline__ float corr_huber(float x) {
  const float a = fabsf(x);
  return a < 1.f ? 0.5f * x * x : a - 0.5f;
}
__device__ __forceinline__ float corr_dhuber(float x) { return fminf(fmaxf(x, -1.f), 1.f); }

// 3 x 3 inverse by cofactors (row-major)
__device__ void corr_inv3(const float* K, float* Ki) {
  const float c00 = K[4] * K[8] - K[5] * K[7], c01 = K[5] * K[6] - K[3] * K[8], c02 = K[3] * K[7] - K[4] * K[6];
  const float det = K[0] * c00 + K[1] * c01 + K[2] * c02;
  Ki[0] = c00 / det; Ki[1] = (K[2] * K[7] - K[1] * K[8]) / det; Ki[2] = (K[1] * K[5] - K[2] * K[4]) / det;
  Ki[3] = c01 / det; Ki[4] = (K[0] * K[8] - K[2] * K[6]) / det; Ki[5] = (K[2] * K[3] - K[0] * K[5]) / det;
  Ki[6] = c02 / det; Ki[7] = (K[1] * K[6] - K[0] * K[7]) / det; Ki[8] = (K[0] * K[4] - K[1] * K[3]) / det;
}

struct CorrGeom {
  float Ks[9], Ko[9], Kis[9], Kio[9];
  float R[2][9], t[2][3];          // [0] = T_self2other, [1] = its rigid inverse
};

// One direction for one row: pixel kp with depth d in image "from" -> re-projected pixel in image "to".
struct CorrProj {
  float kd[3], p[3], uvw[3], inv_w, px, py, z;
};
__device__ __forceinline__ void corr_project(const float* Kinv, const float* K, const float* R, const float* t, float x, float y,
                                             float d, CorrProj& o) {
  for (int a = 0; a < 3; ++a) {
    o.kd[a] = Kinv[a * 3] * x + Kinv[a * 3 + 1] * y + Kinv[a * 3 + 2];
    o.p[a] = o.kd[a] * d;
  }
  float pj[3];
  const float w4 = 1.f + 1e-6f;                         // the homogeneous coordinate of T [p; 1] is exactly 1
  for (int a = 0; a < 3; ++a) pj[a] = (R[a * 3] * o.p[0] + R[a * 3 + 1] * o.p[1] + R[a * 3 + 2] * o.p[2] + t[a]) / w4;
  for (int a = 0; a < 3; ++a) o.uvw[a] = K[a * 3] * pj[0] + K[a * 3 + 1] * pj[1] + K[a * 3 + 2] * pj[2];
  o.inv_w = 1.f / (o.uvw[2] + 1e-6f);
  o.px = o.uvw[0] / (o.uvw[2] + 1e-6f);
  o.py = o.uvw[1] / (o.uvw[2] + 1e-6f);
  o.z = pj[2];
}

// the detached filters of :113-131
__device__ __forceinline__ bool corr_valid(float dx, float dy, float z, float d_to, int pix_chk, float pix_thr, int dep_chk,
                                           float dep_thr) {
  bool ok = true;
  if (pix_chk) ok = ok && (sqrtf(dx * dx + dy * dy) <= pix_thr);
  if (dep_chk) ok = ok && (fabsf(d_to - z) / (d_to + 1e-6f) <= dep_thr);
  return ok;
}

// fixed-order tree over the CORR_T partials of each of n rows of red[n][CORR_T]; red[k][0] holds the sums afterwards
__device__ void corr_tree(float (*red)[CORR_T], int n) {
  __syncthreads();
  for (int o = CORR_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < n; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
}

// depth[p] = [self M | other M] of pass p.  Phase 1 counts the valid rows and sums the weighted Huber terms of each (pass,
// direction); phase 2 re-evaluates every row and writes d loss / d depth and the rows' share of d loss / d T (and of d loss /
// d T^-1), which the tail folds into the two w2c.
__global__ __launch_bounds__(CORR_T) void k_nerf_corres(const float* __restrict__ depth0, const float* __restrict__ depth1, int M,
                                                        const float* __restrict__ pix_s, const float* __restrict__ pix_o,
                                                        const float* __restrict__ conf, const float* __restrict__ K_s,
                                                        const float* __restrict__ K_o, const float* __restrict__ w2c_s,
                                                        const float* __restrict__ w2c_o, int pix_chk, float pix_thr, int dep_chk,
                                                        float dep_thr, float weight, float* __restrict__ loss,
                                                        float* __restrict__ g_depth0, float* __restrict__ g_depth1,
                                                        float* __restrict__ g_w2c) {
  __shared__ CorrGeom G;
  __shared__ float red[24][CORR_T];
  __shared__ float cnt[4];
  const int tid = threadIdx.x;
  if (tid == 0) {
    for (int k = 0; k < 9; ++k) { G.Ks[k] = K_s[k]; G.Ko[k] = K_o[k]; }
    corr_inv3(G.Ks, G.Kis);
    corr_inv3(G.Ko, G.Kio);
    // T = [Ro | to] [Rs^T | -Rs^T ts] ; T^-1 = [RT^T | -RT^T tT]
    float ti[3];
    for (int k = 0; k < 3; ++k) ti[k] = -(w2c_s[k] * w2c_s[3] + w2c_s[4 + k] * w2c_s[7] + w2c_s[8 + k] * w2c_s[11]);
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b)
        G.R[0][a * 3 + b] = w2c_o[a * 4] * w2c_s[b * 4] + w2c_o[a * 4 + 1] * w2c_s[b * 4 + 1] + w2c_o[a * 4 + 2] * w2c_s[b * 4 + 2];
      G.t[0][a] = w2c_o[a * 4] * ti[0] + w2c_o[a * 4 + 1] * ti[1] + w2c_o[a * 4 + 2] * ti[2] + w2c_o[a * 4 + 3];
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) G.R[1][a * 3 + b] = G.R[0][b * 3 + a];
    for (int a = 0; a < 3; ++a)
      G.t[1][a] = -(G.R[0][a] * G.t[0][0] + G.R[0][3 + a] * G.t[0][1] + G.R[0][6 + a] * G.t[0][2]);
  }
  __syncthreads();
  const int np = depth1 ? 2 : 1;

  // ---- phase 1: valid rows and weighted Huber sums per (pass, direction)
  float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = tid; r < M; r += CORR_T) {
    const float xs = pix_s[2 * r], ys = pix_s[2 * r + 1], xo = pix_o[2 * r], yo = pix_o[2 * r + 1], c = conf[r];
#pragma unroll
    for (int p = 0; p < 2; ++p) {          // constant trip count: the partials stay in registers
      if (p >= np) break;
      const float* dp = p ? depth1 : depth0;
      const float ds = dp[r], dop = dp[M + r];
      CorrProj q;
      corr_project(G.Kis, G.Ko, G.R[0], G.t[0], xs, ys, ds, q);
      float dx = q.px - xo, dy = q.py - yo;
      if (corr_valid(dx, dy, q.z, dop, pix_chk, pix_thr, dep_chk, dep_thr)) {
        part[p * 4] += 1.f;
        part[p * 4 + 1] += corr_huber(dx) * c + corr_huber(dy) * c;
      }
      corr_project(G.Kio, G.Ks, G.R[1], G.t[1], xo, yo, dop, q);
      dx = q.px - xs; dy = q.py - ys;
      if (corr_valid(dx, dy, q.z, ds, pix_chk, pix_thr, dep_chk, dep_thr)) {
        part[p * 4 + 2] += 1.f;
        part[p * 4 + 3] += corr_huber(dx) * c + corr_huber(dy) * c;
      }
    }
  }
  for (int k = 0; k < 8; ++k) red[k][tid] = part[k];
  corr_tree(red, 8);
  const float nd = 2.f * (float)np;
  if (tid == 0) {
    float total = 0.f;
    for (int k = 0; k < 2 * np; ++k) total += red[2 * k + 1][0] / (red[2 * k][0] + 1e-6f);
    loss[0] = weight * (total / nd);
    for (int k = 0; k < 4; ++k) cnt[k] = red[2 * k][0];
  }
  __syncthreads();

  // ---- phase 2: gradients.  gsum[0..11] = d/d[R|t] of T, gsum[12..23] = of T^-1 (row-major [R | t] per 3 x 4)
  float gsum[24];
  for (int k = 0; k < 24; ++k) gsum[k] = 0.f;
  for (int r = tid; r < M; r += CORR_T) {
    const float xs = pix_s[2 * r], ys = pix_s[2 * r + 1], xo = pix_o[2 * r], yo = pix_o[2 * r + 1], c = conf[r];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (p >= np) break;
      const float* dp = p ? depth1 : depth0;
      float* gdp = p ? g_depth1 : g_depth0;
      const float d[2] = {dp[r], dp[M + r]};
      for (int dir = 0; dir < 2; ++dir) {
        const float xf = dir ? xo : xs, yf = dir ? yo : ys, xt = dir ? xs : xo, yt = dir ? ys : yo;
        CorrProj q;
        corr_project(dir ? G.Kio : G.Kis, dir ? G.Ks : G.Ko, G.R[dir], G.t[dir], xf, yf, d[dir], q);
        const float dx = q.px - xt, dy = q.py - yt;
        float gd = 0.f;
        if (corr_valid(dx, dy, q.z, d[1 - dir], pix_chk, pix_thr, dep_chk, dep_thr)) {
          const float s = weight / nd / (cnt[p * 2 + dir] + 1e-6f) * c;
          const float gx = s * corr_dhuber(dx), gy = s * corr_dhuber(dy);
          const float guvw[3] = {gx * q.inv_w, gy * q.inv_w, -(gx * q.px + gy * q.py) * q.inv_w};
          const float* K = dir ? G.Ks : G.Ko;
          const float* R = G.R[dir];
          float gq[3];
          for (int b = 0; b < 3; ++b) gq[b] = (K[b] * guvw[0] + K[3 + b] * guvw[1] + K[6 + b] * guvw[2]) / (1.f + 1e-6f);
          float* gs = gsum + 12 * dir;
          for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) gs[a * 4 + b] += gq[a] * q.p[b];
            gs[a * 4 + 3] += gq[a];
          }
          for (int b = 0; b < 3; ++b) gd += (R[b] * gq[0] + R[3 + b] * gq[1] + R[6 + b] * gq[2]) * q.kd[b];
        }
        gdp[dir * M + r] = gd;
      }
    }
  }
  for (int k = 0; k < 24; ++k) red[k][tid] = gsum[k];
  corr_tree(red, 24);
  if (tid == 0) {
    // T^-1 = [RT^T | -RT^T tT]: fold its gradient into T's
    float gR[9], gt[3];
    const float* RT = G.R[0];
    const float* tT = G.t[0];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) gR[a * 3 + b] = red[a * 4 + b][0] + red[12 + b * 4 + a][0] - tT[a] * red[12 + b * 4 + 3][0];
      gt[a] = red[a * 4 + 3][0] - (RT[a * 3] * red[15][0] + RT[a * 3 + 1] * red[19][0] + RT[a * 3 + 2] * red[23][0]);
    }
    // T = [Ro Rs^T | Ro cs + to], cs = -Rs^T ts
    const float *Rs = w2c_s, *Ro = w2c_o;          // row a of the rotation = w2c[a * 4 .. a * 4 + 2]
    float cs[3], gcs[3];
    for (int k = 0; k < 3; ++k) cs[k] = -(Rs[k] * Rs[3] + Rs[4 + k] * Rs[7] + Rs[8 + k] * Rs[11]);
    for (int k = 0; k < 3; ++k) gcs[k] = Ro[k] * gt[0] + Ro[4 + k] * gt[1] + Ro[8 + k] * gt[2];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) {
        // d/dRo[a][b] = sum_k gR[a][k] Rs[k][b] + gt[a] cs[b] ; d/dRs[a][b] = sum_k gR[k][a] Ro[k][b] - ts[a] gcs[b]
        g_w2c[12 + a * 4 + b] = gR[a * 3] * Rs[b] + gR[a * 3 + 1] * Rs[4 + b] + gR[a * 3 + 2] * Rs[8 + b] + gt[a] * cs[b];
        g_w2c[a * 4 + b] = gR[a] * Ro[b] + gR[3 + a] * Ro[4 + b] + gR[6 + a] * Ro[8 + b] - Rs[a * 4 + 3] * gcs[b];
      }
      g_w2c[12 + a * 4 + 3] = gt[a];
      g_w2c[a * 4 + 3] = -(Rs[a * 4] * gcs[0] + Rs[a * 4 + 1] * gcs[1] + Rs[a * 4 + 2] * gcs[2]);
    }
  }
}

extern "C" int pp_nerf_corres_loss(const float* depth0, const float* depth1, int32_t n_pairs, const float* pix_self,
                                   const float* pix_other, const float* conf, const float* K_self, const float* K_other,
                                   const float* w2c_self, const float* w2c_other, int32_t pixel_check, float pixel_thresh,
                                   int32_t depth_check, float depth_thresh, float weight, float* loss, float* g_depth0,
                                   float* g_depth1, float* g_w2c, void* stream) {
  PP_REQUIRE(depth0 && pix_self && pix_other && conf && K_self && K_other && w2c_self && w2c_other && loss && g_depth0 && g_w2c,
             "null pointer");
  PP_REQUIRE((depth1 == nullptr) == (g_depth1 == nullptr), "depth1 and g_depth1 go together");
  PP_REQUIRE(n_pairs > 0, "bad sizes");
  hipLaunchKernelGGL(k_nerf_corres, dim3(1), dim3(CORR_T), 0, pp_stream(stream), depth0, depth1, n_pairs, pix_self, pix_other,
                     conf, K_self, K_other, w2c_self, w2c_other, pixel_check, pixel_thresh, depth_check, depth_thresh, weight,
                     loss, g_depth0, g_depth1, g_w2c);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// rows [0, M) belong to view vs, rows [M, 2M) to view vo: g_c2w[v] += [sum g_ray (x) dir_cam | sum g_center] + the direct
// gradient on w2c[v] moved onto c2w through w2c = [R^T | -R^T t] (the algebra of camera._PoseChain.backward)
__global__ __launch_bounds__(CORR_T) void k_nerf_pair_pose_bwd(const float* __restrict__ g_center, const float* __restrict__ g_ray,
                                                               const float* __restrict__ dir_cam, int M,
                                                               const float* __restrict__ w2c, const float* __restrict__ g_w2c,
                                                               int vs, int vo, float* __restrict__ g_c2w) {
  __shared__ float red[24][CORR_T];
  const int tid = threadIdx.x;
  float part[24];
  for (int k = 0; k < 24; ++k) part[k] = 0.f;
  for (int r = tid; r < 2 * M; r += CORR_T) {
    float* pv = part + (r < M ? 0 : 12);
    const float g0 = g_ray[3 * r], g1 = g_ray[3 * r + 1], g2 = g_ray[3 * r + 2];
    const float d0 = dir_cam[3 * r], d1 = dir_cam[3 * r + 1], d2 = dir_cam[3 * r + 2];
    pv[0] += g0 * d0; pv[1] += g0 * d1; pv[2] += g0 * d2; pv[3] += g_center[3 * r];
    pv[4] += g1 * d0; pv[5] += g1 * d1; pv[6] += g1 * d2; pv[7] += g_center[3 * r + 1];
    pv[8] += g2 * d0; pv[9] += g2 * d1; pv[10] += g2 * d2; pv[11] += g_center[3 * r + 2];
  }
  for (int k = 0; k < 24; ++k) red[k][tid] = part[k];
  corr_tree(red, 24);
  if (tid < 24) {
    const int which = tid / 12, e = tid % 12, a = e / 4, b = e % 4;
    const int v = which ? vo : vs;
    float g = red[tid][0];
    if (g_w2c) {
      const float* P = w2c + v * 12;
      const float* gP = g_w2c + which * 12;
      if (b < 3) {
        const float c = -(P[a] * P[3] + P[4 + a] * P[7] + P[8 + a] * P[11]);      // camera centre = c2w[:, 3]
        g += gP[b * 4 + a] - c * gP[b * 4 + 3];
      } else {
        g += -(P[a] * gP[3] + P[4 + a] * gP[7] + P[8 + a] * gP[11]);
      }
    }
    g_c2w[v * 12 + e] += g;
  }
}

extern "C" int pp_nerf_pair_pose_bwd(const float* g_center, const float* g_ray, const float* dir_cam, int32_t n_pairs,
                                     const float* w2c, const float* g_w2c, int32_t n_views, int32_t view_self,
                                     int32_t view_other, float* g_c2w, void* stream) {
  PP_REQUIRE(g_center && g_ray && dir_cam && w2c && g_c2w, "null pointer");
  PP_REQUIRE(n_pairs > 0 && n_views > 0, "bad sizes");
  PP_REQUIRE(view_self >= 0 && view_self < n_views && view_other >= 0 && view_other < n_views && view_self != view_other,
             "bad view pair");
  hipLaunchKernelGGL(k_nerf_pair_pose_bwd, dim3(1), dim3(CORR_T), 0, pp_stream(stream), g_center, g_ray, dir_cam, n_pairs, w2c,
                     g_w2c, view_self, view_other, g_c2w);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
