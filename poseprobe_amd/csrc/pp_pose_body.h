// Pose forward (se3 -> w2c, c2w, d c2w / d se3): the per-thread body of k_pose_fwd (pp_rays.hip).
#pragma once
#include "pp_common.h"

// ------------------------------------------------------------------------------------------------
// forward-mode dual numbers with 6 tangents (d/d se3) - one thread per view, a few hundred ops.
// ------------------------------------------------------------------------------------------------
// one tangent per thread: thread (view, k) carries d/d se3[k]
struct D6 {
  float v;
  float d;
};
__device__ __forceinline__ D6 d6c(float c) { D6 r; r.v = c; r.d = 0.f; return r; }
__device__ __forceinline__ D6 operator+(const D6& a, const D6& b) { D6 r; r.v = a.v + b.v; r.d = a.d + b.d; return r; }
__device__ __forceinline__ D6 operator-(const D6& a, const D6& b) { D6 r; r.v = a.v - b.v; r.d = a.d - b.d; return r; }
__device__ __forceinline__ D6 operator-(const D6& a) { D6 r; r.v = -a.v; r.d = -a.d; return r; }
__device__ __forceinline__ D6 operator*(const D6& a, const D6& b) { D6 r; r.v = a.v * b.v; r.d = a.d * b.v + a.v * b.d; return r; }
__device__ __forceinline__ D6 operator*(const D6& a, float s) { D6 r; r.v = a.v * s; r.d = a.d * s; return r; }

// Series of lib/camera.py:165-188 written in t = theta^2 (identical polynomial, smooth derivative at 0).
// kind 0: sin(x)/x, 1: (1-cos x)/x^2, 2: (x-sin x)/x^3 ; 11 terms.
static __device__ D6 taylor_t(const D6& t, int kind) {
  D6 ans = d6c(0.f);
  D6 pw = d6c(1.f);
  double denom = 1.0;
  for (int i = 0; i <= 10; ++i) {
    if (kind == 0) { if (i > 0) denom *= (double)((2 * i) * (2 * i + 1)); }
    else if (kind == 1) denom *= (double)((2 * i + 1) * (2 * i + 2));
    else denom *= (double)((2 * i + 2) * (2 * i + 3));
    float c = (float)(((i & 1) ? -1.0 : 1.0) / denom);
    ans = ans + pw * c;
    pw = pw * t;
  }
  return ans;
}

// thread `tidx` = (view, tangent direction): the body of k_pose_fwd, shared with the pose role of k_step_begin (pp_mlp_split.hip)
__device__ __forceinline__ void pose_fwd_elem(int tidx, const float* __restrict__ se3, const float* __restrict__ w2c_init,
                                              const int32_t* __restrict__ refine_mask, int n_views, float* __restrict__ w2c,
                                              float* __restrict__ c2w, float* __restrict__ jac) {
  int v = tidx / 6, kd = tidx - (tidx / 6) * 6;       // view, tangent direction
  if (v >= n_views) return;
  const float* P0 = w2c_init + v * 12;
  D6 Rn[3][3], tn[3];
  bool refine = (refine_mask == nullptr) || refine_mask[v] != 0;
  if (!refine) {
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Rn[i][j] = d6c(P0[i * 4 + j]); tn[i] = d6c(P0[i * 4 + 3]); }
  } else {
    D6 w[3], u[3];
    for (int k = 0; k < 3; ++k) {
      w[k] = d6c(se3[v * 6 + k]); w[k].d = (kd == k) ? 1.f : 0.f;
      u[k] = d6c(se3[v * 6 + 3 + k]); u[k].d = (kd == 3 + k) ? 1.f : 0.f;
    }
    D6 t = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    D6 A = taylor_t(t, 0), B = taylor_t(t, 1), C = taylor_t(t, 2);
    D6 z = d6c(0.f);
    D6 wx[3][3] = {{z, -w[2], w[1]}, {w[2], z, -w[0]}, {-w[1], w[0], z}};
    D6 wx2[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) wx2[i][j] = wx[i][0] * wx[0][j] + wx[i][1] * wx[1][j] + wx[i][2] * wx[2][j];
    D6 R[3][3], Vm[3][3], tr[3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
      D6 eye = d6c(i == j ? 1.f : 0.f);
      R[i][j] = eye + A * wx[i][j] + B * wx2[i][j];
      Vm[i][j] = eye + B * wx[i][j] + C * wx2[i][j];
    }
    for (int i = 0; i < 3; ++i) tr[i] = Vm[i][0] * u[0] + Vm[i][1] * u[1] + Vm[i][2] * u[2];
    // compose_pair(pose_a = refine, pose_b = init): R = R_b R_a ; t = R_b t_a + t_b   (camera.py:92-99)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rn[i][j] = R[0][j] * P0[i * 4 + 0] + R[1][j] * P0[i * 4 + 1] + R[2][j] * P0[i * 4 + 2];
      tn[i] = tr[0] * P0[i * 4 + 0] + tr[1] * P0[i * 4 + 1] + tr[2] * P0[i * 4 + 2] + d6c(P0[i * 4 + 3]);
    }
  }
  // invert: R^T, -R^T t (camera.py:76-82)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      if (kd == 0) { w2c[v * 12 + i * 4 + j] = Rn[i][j].v; c2w[v * 12 + i * 4 + j] = Rn[j][i].v; }
      jac[(v * 12 + i * 4 + j) * 6 + kd] = Rn[j][i].d;
    }
    D6 ti = -(Rn[0][i] * tn[0] + Rn[1][i] * tn[1] + Rn[2][i] * tn[2]);
    if (kd == 0) { w2c[v * 12 + i * 4 + 3] = tn[i].v; c2w[v * 12 + i * 4 + 3] = ti.v; }
    jac[(v * 12 + i * 4 + 3) * 6 + kd] = ti.d;
  }
}
