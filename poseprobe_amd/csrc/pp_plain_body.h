// Device code of the plain-template geometry forward (use_deform=False), shared by the render path's kernels
// (pp_forward_variants.hip) and the mesh colour kernel (pp_mesh_color.hip): the 32-node stencil of the raw sdf template, its
// mapping in registers and plain_forward, the interpolated value and central-difference gradient of one sample.
#pragma once
#include "pp_common.h"

namespace {

// corner c = dx * 4 + dy * 2 + dz; BIT[a] is the bit of axis a in c
__device__ __forceinline__ constexpr int axis_bit(int a) { return a == 0 ? 4 : (a == 1 ? 2 : 1); }

struct PlainCell {
  float w[3][2];   // weight of the lower / upper corner along each axis
  int idx[3][4];   // nodes base - 1 .. base + 2 along each axis, clamped to the grid
  bool cd[3][2];   // node base + d has a central difference along the axis (1 <= node <= size - 2), else the component is 0
  float gm[3];     // d(clipped coordinate) / d(coordinate): 0 where the border padding clipped it (u <= 0 or u >= size - 1)
};

__device__ __forceinline__ void plain_setup(const SceneDev& sc, const float p[3], PlainCell& t) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float top = (float)(sc.sz[a] - 1);
    float u = pp_grid_u(p[a], sc.mn[a], sc.mx[a], sc.sz[a]);
    t.gm[a] = (u > 0.f && u < top) ? 1.f : 0.f;
    u = fminf(fmaxf(u, 0.f), top);              // padding_mode='border' (a NaN coordinate lands on node 0)
    const float f = floorf(u);
    t.w[a][1] = pp_sub(u, f);
    t.w[a][0] = pp_sub(pp_add(f, 1.f), u);
    const int b = (int)f;
#pragma unroll
    for (int k = 0; k < 4; ++k) t.idx[a][k] = min(max(b - 1 + k, 0), sc.sz[a] - 1);
#pragma unroll
    for (int d = 0; d < 2; ++d) t.cd[a][d] = (b + d >= 1) && (b + d <= sc.sz[a] - 2);
  }
}

// V[0][c]: the corner itself; V[1 + a][c]: its neighbour one node further OUT along axis a (base - 1 below a lower corner, base + 2
// above an upper one).  The neighbour one node further IN is the corner c ^ bit(a).
__device__ __forceinline__ void plain_gather(const SceneDev& sc, const float* __restrict__ grid, const PlainCell& t, float V[4][8]) {
  const size_t Y = sc.sz[1], Z = sc.sz[2];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      int k[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int d = (c & axis_bit(a)) ? 1 : 0;
        k[a] = (g == 1 + a) ? (d ? 3 : 0) : 1 + d;
      }
      V[g][c] = grid[((size_t)t.idx[0][k[0]] * Y + t.idx[1][k[1]]) * Z + t.idx[2][k[2]]];
    }
  }
}

__device__ __forceinline__ float corner_weight(const PlainCell& t, int c) {
  return (t.w[0][(c >> 2) & 1] * t.w[1][(c >> 1) & 1]) * t.w[2][c & 1];
}

struct PlainFwd {
  float sdf, grad[3], D[3][8];
  float cosv, ic, pc, nc, num, den, a_un;
};

// S: raw template values (plain_gather), G: the same mapped.  The central difference of node n along a axis is
// (G[n + 1] - G[n - 1]) / 2 / voxel_size in this order (neus_sdf_gradient), zero on the two boundary planes of that axis.
__device__ __forceinline__ void plain_forward(const SceneDev& sc, const PlainCell& t, const float A, const float B, const float S[4][8],
                                              const float v[3], const float inv_s, float G[4][8], PlainFwd& o) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int c = 0; c < 8; ++c) G[g][c] = A * (pp_sigmoid(B * S[g][c]) - 0.5f);
  o.sdf = 0.f;
  o.grad[0] = o.grad[1] = o.grad[2] = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float w = corner_weight(t, c);
    o.sdf += G[0][c] * w;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int d = (c & axis_bit(a)) ? 1 : 0;
      const float out = G[1 + a][c], in = G[0][c ^ axis_bit(a)];
      const float diff = d ? pp_sub(out, in) : pp_sub(in, out);
      o.D[a][c] = t.cd[a][d] ? pp_div(pp_mul(diff, 0.5f), sc.voxel) : 0.f;
      o.grad[a] += o.D[a][c] * w;
    }
  }
  // NeuS alpha, use_mid, cos_anneal_ratio = 1: the expressions of the default geometry kernel (pp_geometry.hip)
  const float dist = pp_mul(sc.stepsize, sc.voxel);
  o.cosv = v[0] * o.grad[0] + v[1] * o.grad[1] + v[2] * o.grad[2];
  o.ic = fminf(o.cosv, 0.f);
  const float off = (o.ic * dist) * 0.5f;
  const float nxt = o.sdf + off, prv = o.sdf - off;
  o.pc = pp_sigmoid(prv * inv_s);
  o.nc = pp_sigmoid(nxt * inv_s);
  o.num = (o.pc - o.nc) + 1e-5f;
  o.den = o.pc + 1e-5f;
  o.a_un = o.num / o.den;
}

}  // namespace
