// Vertex attributes of an extracted mesh: the render path's colour stage with the ray removed.  One launch between
// the warp net and the rgbnet turns n vertices into their unit normals and their rows of the rgbnet's input:
//   g      = d sdf / d p - geo_forward's `grad` through the warp Jacobian (pp_geometry_body.h), or, without the warp net,
//            plain_forward's interpolated central differences (pp_plain_body.h);
//   normal = g / (|g| + 1e-5), viewdir = -normal: the vertex seen head-on;
//   row    = [k0(p) | PE_pos(p) | PE_view(viewdir) | normal | 0 x 7], the <12, 5, 1> layout of pp_color_body.h.
// The device code is the render path's own: nothing is restated here, the view embedding takes the normal from registers where
// the render path reads viewdirs[ray_id].  Forward only: no ray_id, no alpha, no step, no atomics, no workspace.
//
// Lane layout: one lane per vertex, every k0 corner as 3 x 16-byte loads, the layout of the render path's colour kernel.  A
// vertex reads 8 x 48 B of k0 and 8 (32 without the warp net) template nodes; marching cubes emits the vertices in lattice
// order, so the 64 vertices of a wavefront sit on neighbouring lattice edges and share most of their cells - the gathers of a
// wavefront fall into a few runs along z (k0 is [X,Y,Z,C]: the two z corners of a cell pair are 96 contiguous bytes) and hit in
// L1 / L2 after the first lane's miss.  Spreading a vertex over several lanes (a corner per lane) would buy wider coalescing of
// one vertex's own 384 B at the price of cross-lane sums in another order than the render path's: the rows would no longer be
// the bits that path gives, and the loads already arrive as full 16-byte pieces.
#include "pp_common.h"
#include "pp_k0_tri.h"
#include "pp_color_body.h"
#include "pp_geometry_body.h"
#include "pp_plain_body.h"

namespace {

constexpr int VERTEX_THREADS = 256;

template <bool DEFORM>
__global__ __launch_bounds__(VERTEX_THREADS) void k_vertex_feat(SceneDev sc, const float* __restrict__ grid,
                                                                const float* __restrict__ sdf_ab, const float* __restrict__ k0,
                                                                const float* __restrict__ pts, const float* __restrict__ warp_out,
                                                                const float* __restrict__ pe_w, int n, float* __restrict__ normal,
                                                                float* __restrict__ feat) {
  const int m = blockIdx.x * VERTEX_THREADS + threadIdx.x;
  if (m >= n) return;
  const size_t m3 = (size_t)m * 3;
  const float p[3] = {pts[m3], pts[m3 + 1], pts[m3 + 2]};
  const float zero[3] = {0.f, 0.f, 0.f};        // no ray: the NeuS alpha of the shared forward is dead code here
  float g[3];
  if (DEFORM) {
    const MapAB mp = map_ab(sdf_ab);
    float wo[16];
    const float4* w4 = reinterpret_cast<const float4*>(warp_out + (size_t)m * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) { float4 t = w4[i]; wo[i * 4] = t.x; wo[i * 4 + 1] = t.y; wo[i * 4 + 2] = t.z; wo[i * 4 + 3] = t.w; }
    float scl[3];
    for (int k = 0; k < 3; ++k) scl[k] = (float)(sc.sz[k] - 1) / (sc.mx[k] - sc.mn[k]);
    Tri tq, tp;
    float Sq[8], Sp[8], Gq[8], Gp[8];
    GeoFwd o;
    geo_forward(sc, grid, mp, p, wo, zero, 0.f, scl, tq, Sq, tp, Sp, Gq, Gp, o);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = o.grad[k];
  } else {
    const float A = pp_softplus10(sdf_ab[0]), B = pp_softplus10(sdf_ab[1]);
    PlainCell t;
    plain_setup(sc, p, t);
    float S[4][8], G[4][8];
    plain_gather(sc, grid, t, S);
    PlainFwd o;
    plain_forward(sc, t, A, B, S, zero, 0.f, G, o);
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = o.grad[k];
  }
  float nrm[3];
  color_feat_fwd_body<12, 5, 1, true, true>(m, sc, k0, pts, nullptr, nullptr, g, pe_w, nullptr, n, feat, nrm);
#pragma unroll
  for (int a = 0; a < 3; ++a) normal[m3 + a] = nrm[a];
}

}  // namespace

extern "C" int pp_vertex_feat(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* k0_cl, const float* pts,
                              const float* warp_out, const float* pe_w, int32_t n, float* normal, float* feat, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && k0_cl && pe_w, "null pointer");
  PP_REQUIRE(n >= 0 && n <= (1 << 29), "n must be in [0, 2^29] (the shared bodies index rows with 32-bit 3 m)");
  if (!(sc->k0_dim == 12 && sc->pos_pe == 5 && sc->view_pe == 1)) {
    pp_set_error("%s: only the shipped colour-stage shape (k0_dim = 12, pos_pe = 5, view_pe = 1) is covered", __func__);
    return PP_ERR_UNSUPPORTED;
  }
  PP_REQUIRE(sc->size[0] >= 2 && sc->size[1] >= 2 && sc->size[2] >= 2, "the template needs two nodes along every axis");
  if (n == 0) return PP_OK;                     // nothing to do: no launch
  PP_REQUIRE(pts && normal && feat, "null pointer");
  const SceneDev sd = pp_scene_dev(sc);
  const dim3 grid(pp_div_up(n, VERTEX_THREADS)), block(VERTEX_THREADS);
  if (warp_out)
    hipLaunchKernelGGL(k_vertex_feat<true>, grid, block, 0, pp_stream(stream), sd, sdf_grid, sdf_ab, k0_cl, pts, warp_out, pe_w, n,
                       normal, feat);
  else
    hipLaunchKernelGGL(k_vertex_feat<false>, grid, block, 0, pp_stream(stream), sd, sdf_grid, sdf_ab, k0_cl, pts,
                       (const float*)nullptr, pe_w, n, normal, feat);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
