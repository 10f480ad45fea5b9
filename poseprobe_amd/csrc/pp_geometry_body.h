// Device code of the deformed-template geometry forward, shared by the render path's kernels (pp_geometry.hip) and the mesh
// colour kernel (pp_mesh_color.hip): the custom trilinear stencil of the sdf template, the alpha / beta mapping of its corner
// values in registers and geo_forward, one sample's forward from its point and its row of the warp net's output.
#pragma once
#include "pp_common.h"

struct Tri {
  float w0[3], w1[3];
  int i0[3], i1[3];
};

__device__ __forceinline__ void tri_setup(const SceneDev& sc, const float p[3], Tri& t) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float u = pp_grid_u(p[a], sc.mn[a], sc.mx[a], sc.sz[a]);
    float f = floorf(u);
    t.w1[a] = pp_sub(u, f);                 // weight of the +1 corner, from the UNCLAMPED floor (voxurf_coarse.py:589-596)
    t.w0[a] = pp_sub(pp_add(f, 1.f), u);
    float fc = fminf(fmaxf(f, -2.f), (float)sc.sz[a]);
    int i = (int)fc;
    t.i0[a] = min(max(i, 0), sc.sz[a] - 1);  // indices clamped (voxurf_coarse.py:598-629)
    t.i1[a] = min(max(i + 1, 0), sc.sz[a] - 1);
  }
}

// raw corner values, order c = dx*4 + dy*2 + dz
__device__ __forceinline__ void tri_gather(const SceneDev& sc, const float* __restrict__ grid, const Tri& t, float S[8]) {
  const int Y = sc.sz[1], Z = sc.sz[2];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int ix = (c & 4) ? t.i1[0] : t.i0[0];
    int iy = (c & 2) ? t.i1[1] : t.i0[1];
    int iz = (c & 1) ? t.i1[2] : t.i0[2];
    size_t flat = ((size_t)ix * Y + iy) * Z + iz;
    if (sc.flat_f32) {
      // the reference's fp32 index arithmetic, left to right: ((x * Z) * Y + y * Z) + z, each step rounded to fp32, then
      // truncated (.long()); clamped to the grid (the reference's gather would fault on the one index that rounds past it)
      const float f = __fadd_rn(__fadd_rn(__fmul_rn(__fmul_rn((float)ix, (float)Z), (float)Y), __fmul_rn((float)iy, (float)Z)), (float)iz);
      const size_t total = (size_t)sc.sz[0] * Y * Z;
      flat = (size_t)(long long)f;
      if (flat >= total) flat = total - 1;
    }
    S[c] = grid[flat];
  }
}

struct MapAB {
  float A, B, dA, dB;  // softplus10(alpha_raw), softplus10(beta_raw) and their derivatives
};
__device__ __forceinline__ MapAB map_ab(const float* __restrict__ sdf_ab) {
  MapAB m;
  m.A = pp_softplus10(sdf_ab[0]); m.B = pp_softplus10(sdf_ab[1]);
  m.dA = pp_dsoftplus10(sdf_ab[0]); m.dB = pp_dsoftplus10(sdf_ab[1]);
  return m;
}

__device__ __forceinline__ float tri_value(const Tri& t, const float G[8]) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float wx = (c & 4) ? t.w1[0] : t.w0[0], wy = (c & 2) ? t.w1[1] : t.w0[1], wz = (c & 1) ? t.w1[2] : t.w0[2];
    v += G[c] * ((wz * wy) * wx);
  }
  return v;
}

// gradient in voxel units (du) and the three mixed second derivatives
__device__ __forceinline__ void tri_grad(const Tri& t, const float G[8], float g[3], float h[3]) {
  g[0] = g[1] = g[2] = 0.f;
  h[0] = h[1] = h[2] = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float sx = (c & 4) ? 1.f : -1.f, sy = (c & 2) ? 1.f : -1.f, sz = (c & 1) ? 1.f : -1.f;
    float wx = (c & 4) ? t.w1[0] : t.w0[0], wy = (c & 2) ? t.w1[1] : t.w0[1], wz = (c & 1) ? t.w1[2] : t.w0[2];
    g[0] += G[c] * (sx * wy * wz);
    g[1] += G[c] * (wx * sy * wz);
    g[2] += G[c] * (wx * wy * sz);
    h[0] += G[c] * (sx * sy * wz);  // d2/dxdy
    h[1] += G[c] * (sx * wy * sz);  // d2/dxdz
    h[2] += G[c] * (wx * sy * sz);  // d2/dydz
  }
}

struct GeoFwd {
  float q[3], gq[3], A[3][3], Jc[3], corr, vq, vp, sdf, grad[3];
  float cosv, ic, pc, nc, num, den, a_un;
};

__device__ __forceinline__ void geo_forward(const SceneDev& sc, const float* __restrict__ grid, const MapAB& mp,
                                            const float p[3], const float wo[16], const float v[3], float inv_s,
                                            const float scl[3], Tri& tq, float Sq[8], Tri& tp, float Sp[8],
                                            float Gq[8], float Gp[8], GeoFwd& o) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o.q[k] = p[k] + wo[k];
  o.corr = wo[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o.A[i][j] = (i == j ? 1.f : 0.f) + wo[(1 + i) * 4 + j];
    o.Jc[i] = wo[(1 + i) * 4 + 3];
  }
  tri_setup(sc, o.q, tq);
  tri_gather(sc, grid, tq, Sq);
  tri_setup(sc, p, tp);
  tri_gather(sc, grid, tp, Sp);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    Gq[c] = mp.A * (pp_sigmoid(mp.B * Sq[c]) - 0.5f);
    Gp[c] = mp.A * (pp_sigmoid(mp.B * Sp[c]) - 0.5f);
  }
  o.vq = tri_value(tq, Gq);
  o.vp = tri_value(tp, Gp);
  float gu[3], hu[3];
  tri_grad(tq, Gq, gu, hu);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.gq[k] = gu[k] * scl[k];
  o.sdf = o.vq + o.corr;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.grad[i] = o.A[i][0] * o.gq[0] + o.A[i][1] * o.gq[1] + o.A[i][2] * o.gq[2] + o.Jc[i];
  // NeuS alpha, use_mid, cos_anneal_ratio = 1
  float dist = pp_mul(sc.stepsize, sc.voxel);
  o.cosv = v[0] * o.grad[0] + v[1] * o.grad[1] + v[2] * o.grad[2];
  o.ic = fminf(o.cosv, 0.f);
  float off = (o.ic * dist) * 0.5f;
  float nxt = o.sdf + off, prv = o.sdf - off;
  o.pc = pp_sigmoid(prv * inv_s);
  o.nc = pp_sigmoid(nxt * inv_s);
  o.num = (o.pc - o.nc) + 1e-5f;
  o.den = o.pc + 1e-5f;
  o.a_un = o.num / o.den;
}
