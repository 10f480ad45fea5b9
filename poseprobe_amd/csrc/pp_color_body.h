// Colour-feature bodies shared by their stand-alone kernels (pp_color.hip) and by the launches that carry them as work-group roles
// beside a geometry kernel (pp_geometry.hip).
#pragma once
#include "pp_common.h"
#include "pp_k0_tri.h"

__device__ __forceinline__ float pp_norm3c(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

// sample m of the feature builder.  NORMAL = false: columns [0, C + 6 + 6 Lp + 6 Lv) only (54 for the <12, 5, 1> layout) - the normal
// columns and the zero padding are written by the geometry role of the same launch (pp_geometry.hip, k_geometry_color_fwd);
// `gradient` is not read then.
// HEADON = true (the mesh colour kernel, pp_mesh_color.hip: a vertex seen head-on, no ray): `gradient` is this sample's own g[3], not
// a table indexed by m; the view direction is minus the normal g / (|g| + 1e-5) formed here in registers, viewdirs / ray_id / count
// are not read (every m < capacity is live) and the normal is handed back in normal_out[3].  HEADON = false compiles to the code it
// compiled to before the parameter existed.
template <int TC, int TLP, int TLV, bool NORMAL, bool HEADON = false>
__device__ __forceinline__ void color_feat_fwd_body(int m, const SceneDev& sc, const float* __restrict__ k0,
                                                    const float* __restrict__ pts, const float* __restrict__ viewdirs,
                                                    const int32_t* __restrict__ ray_id, const float* __restrict__ gradient,
                                                    const float* __restrict__ pe_w, const int32_t* __restrict__ count,
                                                    int capacity, float* __restrict__ feat, float* normal_out = nullptr) {
  static_assert(!HEADON || NORMAL, "a head-on row carries its normal");
  int M = HEADON ? capacity : min(count[0], capacity);
  if (m >= M) return;
  float f[PP_FEAT_LD];
#pragma unroll
  for (int i = 0; i < PP_FEAT_LD; ++i) f[i] = 0.f;
  float p[3] = {pts[m * 3], pts[m * 3 + 1], pts[m * 3 + 2]};
  K0Tri t;
  k0_setup(sc, p, t);
  const int C = TC ? TC : sc.C;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    size_t off; float w;
    if (k0_corner(sc, t, c, off, w)) {
      const float4* src = reinterpret_cast<const float4*>(k0 + off);
#pragma unroll
      for (int q = 0; q < C / 4; ++q) {
        float4 v = src[q];
        f[q * 4 + 0] += v.x * w; f[q * 4 + 1] += v.y * w; f[q * 4 + 2] += v.z * w; f[q * 4 + 3] += v.w * w;
      }
    }
  }
  int o = C;
  const int Lp = TLP ? TLP : sc.Lp, Lv = TLV ? TLV : sc.Lv;
  // xyz embedding: [t(3) | w_k sin(2^k t_a) (a major, k minor) | w_k cos(...)]
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float ta = pp_div(pp_sub(p[a], sc.mn[a]), pp_sub(sc.mx[a], sc.mn[a]));
    f[o + a] = ta;
    float fr = 1.f;
#pragma unroll
    for (int k = 0; k < Lp; ++k) {
      float ang = ta * fr, s, c;
      sincosf(ang, &s, &c);
      f[o + 3 + a * Lp + k] = s * pe_w[k];
      f[o + 3 + 3 * Lp + a * Lp + k] = c * pe_w[k];
      fr *= 2.f;
    }
  }
  o += 3 + 6 * Lp;
  float nrm[3];
  if (HEADON) {
    float gn = pp_norm3c(gradient[0], gradient[1], gradient[2]) + 1e-5f;
    for (int a = 0; a < 3; ++a) normal_out[a] = nrm[a] = gradient[a] / gn;
  }
  int r = HEADON ? 0 : ray_id[m];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float va = HEADON ? -nrm[a] : viewdirs[r * 3 + a];
    f[o + a] = va;
    float fr = 1.f;
#pragma unroll
    for (int k = 0; k < Lv; ++k) {
      float ang = va * fr, s, c;
      sincosf(ang, &s, &c);
      f[o + 3 + a * Lv + k] = s * pe_w[Lp + k];
      f[o + 3 + 3 * Lv + a * Lv + k] = c * pe_w[Lp + k];
      fr *= 2.f;
    }
  }
  o += 3 + 6 * Lv;
  float4* dst = reinterpret_cast<float4*>(feat + (size_t)m * PP_FEAT_LD);
  if (HEADON) {
    for (int a = 0; a < 3; ++a) f[o + a] = nrm[a];
#pragma unroll
    for (int q = 0; q < PP_FEAT_LD / 4; ++q) dst[q] = make_float4(f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]);
  } else if (NORMAL) {
    float g[3] = {gradient[m * 3], gradient[m * 3 + 1], gradient[m * 3 + 2]};
    float gn = pp_norm3c(g[0], g[1], g[2]) + 1e-5f;
    for (int a = 0; a < 3; ++a) f[o + a] = g[a] / gn;
#pragma unroll
    for (int q = 0; q < PP_FEAT_LD / 4; ++q) dst[q] = make_float4(f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]);
  } else {
    // fixed layout only: o = 54, columns 52 - 55 share one float4 with the normal: that piece goes out as scalar stores from each side
    static_assert(NORMAL || (TC == 12 && TLP == 5 && TLV == 1), "the split feature row is laid out for C = 12, Lp = 5, Lv = 1");
#pragma unroll
    for (int q = 0; q < 13; ++q) dst[q] = make_float4(f[q * 4], f[q * 4 + 1], f[q * 4 + 2], f[q * 4 + 3]);
    feat[(size_t)m * PP_FEAT_LD + 52] = f[52];
    feat[(size_t)m * PP_FEAT_LD + 53] = f[53];
  }
}
