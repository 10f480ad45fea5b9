// Geometry stage, one thread per sample: deformed / undeformed SDF lookup with the alpha/beta mapping applied to the
// 8 corner values in registers (the mapped G^3 grid of lib/voxurf_coarse.py:946-949 is never written), analytic
// spatial gradient + mixed second derivatives of the trilinear interpolant (replaces the autograd passes of
// :968-984), NeuS alpha (:483-519).  The sdf template is [X][Y][Z] fp32 (4 B gathers, L2/Infinity-Cache resident:
// 3.5 MB at 96^3, 16 MB at 160^3).
#include "pp_common.h"
#include "pp_ordered.h"
#include "pp_color_body.h"
#include "pp_geometry_body.h"

// sample m of the geometry forward.  feat != nullptr (k_geometry_color_fwd): the normal columns 54 - 56 and the zero padding
// 57 - 63 of the rgbnet's input row are written here, with the colour kernel's own expression, beside the colour role that
// writes columns 0 - 53; columns 52 - 55 share one float4: that piece goes out as scalar stores from each side.
__device__ __forceinline__ void geometry_fwd_body(int m, const SceneDev& sc, const float* __restrict__ grid,
                                                  const float* __restrict__ sdf_ab, const float* __restrict__ pts,
                                                  const float* __restrict__ warp_out, const float* __restrict__ viewdirs,
                                                  const int32_t* __restrict__ ray_id, const int32_t* __restrict__ count,
                                                  int capacity, float inv_s, float* __restrict__ alpha,
                                                  float* __restrict__ gradient, float* __restrict__ sdf_final,
                                                  float* __restrict__ sdf_deform, float* __restrict__ grad_deform,
                                                  float* __restrict__ feat) {
  int M = min(count[0], capacity);
  if (m >= M) return;
  MapAB mp = map_ab(sdf_ab);
  float p[3] = {pts[m * 3], pts[m * 3 + 1], pts[m * 3 + 2]};
  float wo[16];
  const float4* w4 = reinterpret_cast<const float4*>(warp_out + (size_t)m * 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) { float4 t = w4[i]; wo[i * 4] = t.x; wo[i * 4 + 1] = t.y; wo[i * 4 + 2] = t.z; wo[i * 4 + 3] = t.w; }
  int r = ray_id[m];
  float v[3] = {viewdirs[r * 3], viewdirs[r * 3 + 1], viewdirs[r * 3 + 2]};
  float scl[3];
  for (int k = 0; k < 3; ++k) scl[k] = (float)(sc.sz[k] - 1) / (sc.mx[k] - sc.mn[k]);
  Tri tq, tp;
  float Sq[8], Sp[8], Gq[8], Gp[8];
  GeoFwd o;
  geo_forward(sc, grid, mp, p, wo, v, inv_s, scl, tq, Sq, tp, Sp, Gq, Gp, o);
  alpha[m] = fminf(fmaxf(o.a_un, 0.f), 1.f);
  for (int k = 0; k < 3; ++k) gradient[m * 3 + k] = o.grad[k];
  if (sdf_final) sdf_final[m] = o.sdf;
  if (sdf_deform) sdf_deform[m] = o.sdf - o.vp;
  if (grad_deform)
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) grad_deform[m * 9 + i * 3 + j] = o.A[i][j];
  if (feat) {
    const float gn = pp_norm3c(o.grad[0], o.grad[1], o.grad[2]) + 1e-5f;
    float* row = feat + (size_t)m * PP_FEAT_LD;
    row[54] = o.grad[0] / gn;
    row[55] = o.grad[1] / gn;
    float4* r4 = reinterpret_cast<float4*>(row);
    r4[14] = make_float4(o.grad[2] / gn, 0.f, 0.f, 0.f);
    r4[15] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__global__ __launch_bounds__(256) void k_geometry_fwd(SceneDev sc, const float* __restrict__ grid,
                                                      const float* __restrict__ sdf_ab, const float* __restrict__ pts,
                                                      const float* __restrict__ warp_out,
                                                      const float* __restrict__ viewdirs,
                                                      const int32_t* __restrict__ ray_id,
                                                      const int32_t* __restrict__ count, int capacity, float inv_s,
                                                      float* __restrict__ alpha, float* __restrict__ gradient,
                                                      float* __restrict__ sdf_final, float* __restrict__ sdf_deform,
                                                      float* __restrict__ grad_deform) {
  geometry_fwd_body(blockIdx.x * blockDim.x + threadIdx.x, sc, grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s,
                    alpha, gradient, sdf_final, sdf_deform, grad_deform, nullptr);
}

// Geometry forward and colour lookup in ONE launch: only the three normal columns of the rgbnet's input need the
// geometry; the k0 gather, both encodings and their stores need pts / viewdirs / ray_id alone.  Work-groups alternate:
// even = geometry role, odd = colour role, each over samples [256 (blockIdx / 2), ...) - the live work-groups of both roles sit
// at the front of the grid and run side by side.
__global__ __launch_bounds__(256) void k_geometry_color_fwd(SceneDev sc, const float* __restrict__ grid,
                                                            const float* __restrict__ sdf_ab, const float* __restrict__ pts,
                                                            const float* __restrict__ warp_out,
                                                            const float* __restrict__ viewdirs,
                                                            const int32_t* __restrict__ ray_id,
                                                            const int32_t* __restrict__ count, int capacity, float inv_s,
                                                            float* __restrict__ alpha, float* __restrict__ gradient,
                                                            float* __restrict__ sdf_final, float* __restrict__ sdf_deform,
                                                            float* __restrict__ grad_deform, const float* __restrict__ k0,
                                                            const float* __restrict__ pe_w, float* feat) {
  const int m = (blockIdx.x >> 1) * 256 + threadIdx.x;
  if (blockIdx.x & 1)
    color_feat_fwd_body<12, 5, 1, false>(m, sc, k0, pts, viewdirs, ray_id, nullptr, pe_w, count, capacity, feat);
  else
    geometry_fwd_body(m, sc, grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient, sdf_final,
                      sdf_deform, grad_deform, feat);
}

// PRIORS: the sample-level regularisers of object_losses (lib/losses.py:6-23: eikonal, deformation-Jacobian norm,
// |correction|, |sdf_deform|) are differentiated right here from the recomputed forward instead of by a separate kernel
// that writes g_grad_deform / g_correction / g_sdf_deform to HBM first (pp_loss_samples); same expressions, same
// order of additions, so the two routes are bit-identical.
#define GEO_BWD_THREADS 512
static_assert(GEO_BWD_THREADS == ORD_GEO_THREADS, "the ordered-flush workspace is sized by this block size");
template <bool PRIORS>
__global__ __launch_bounds__(GEO_BWD_THREADS) void k_geometry_bwd(
    SceneDev sc, const float* __restrict__ grid, const float* __restrict__ sdf_ab, const float* __restrict__ pts,
    const float* __restrict__ warp_out, const float* __restrict__ viewdirs, const int32_t* __restrict__ ray_id,
    const int32_t* __restrict__ count, int capacity, float inv_s, const float* __restrict__ g_alpha,
    const float* __restrict__ g_gradient, const float* __restrict__ g_sdf_final, const float* __restrict__ g_sdf_deform,
    const float* __restrict__ g_grad_deform, const float* __restrict__ g_correction, int accumulate,
    float* __restrict__ warp_out_grad, float* __restrict__ pts_grad, float* __restrict__ vgrad_s,
    float* __restrict__ sdf_ab_grad, float w_eik, float w_dyn, float ls, float* __restrict__ loss_out,
    const float* __restrict__ batch_norm, float* __restrict__ part) {
  __shared__ float red[6][GEO_BWD_THREADS / 64];
  int m = blockIdx.x * blockDim.x + threadIdx.x;
  int M = min(count[0], capacity);
  float ga_sum = 0.f, gb_sum = 0.f;
  float l_eik = 0.f, l_gd = 0.f, l_c = 0.f, l_sd = 0.f;
  float invM = M > 0 ? 1.f / (float)M : 0.f;
  if (PRIORS && batch_norm) invM = batch_norm[1] > 0.f ? 1.f / batch_norm[1] : 0.f;   // union batch's sample count / world size
  if (m < M) {
    MapAB mp = map_ab(sdf_ab);
    float p[3] = {pts[m * 3], pts[m * 3 + 1], pts[m * 3 + 2]};
    float wo[16];
    const float4* w4 = reinterpret_cast<const float4*>(warp_out + (size_t)m * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) { float4 t = w4[i]; wo[i * 4] = t.x; wo[i * 4 + 1] = t.y; wo[i * 4 + 2] = t.z; wo[i * 4 + 3] = t.w; }
    int r = ray_id[m];
    float v[3] = {viewdirs[r * 3], viewdirs[r * 3 + 1], viewdirs[r * 3 + 2]};
    float scl[3];
    for (int k = 0; k < 3; ++k) scl[k] = (float)(sc.sz[k] - 1) / (sc.mx[k] - sc.mn[k]);
    Tri tq, tp;
    float Sq[8], Sp[8], Gq[8], Gp[8];
    GeoFwd o;
    geo_forward(sc, grid, mp, p, wo, v, inv_s, scl, tq, Sq, tp, Sp, Gq, Gp, o);
    float dist = pp_mul(sc.stepsize, sc.voxel);
    // ---- alpha backward (clip passes the gradient on the closed interval, as torch.clamp)
    float ga = g_alpha ? g_alpha[m] : 0.f;
    if (!(o.a_un >= 0.f && o.a_un <= 1.f)) ga = 0.f;
    float n_bar = ga / o.den;
    float d_bar = -ga * o.num / (o.den * o.den);
    float pc_bar = n_bar + d_bar, nc_bar = -n_bar;
    float prv_bar = pc_bar * o.pc * (1.f - o.pc) * inv_s;
    float nxt_bar = nc_bar * o.nc * (1.f - o.nc) * inv_s;
    float sdf_bar = prv_bar + nxt_bar + (g_sdf_final ? g_sdf_final[m] : 0.f);
    float ic_bar = (nxt_bar - prv_bar) * (dist * 0.5f);
    float cos_bar = (o.cosv < 0.f) ? ic_bar : 0.f;
    float gg[3], vb[3];
    float eik[3] = {0.f, 0.f, 0.f}, gdef_bar[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, corr_bar = 0.f, sdef_bar = 0.f;
    if (PRIORS) {
      const float gn = sqrtf(o.grad[0] * o.grad[0] + o.grad[1] * o.grad[1] + o.grad[2] * o.grad[2]);
      const float e = gn - 1.f;
      l_eik = fabsf(e);
      const float sg = (e > 0.f) ? 1.f : (e < 0.f ? -1.f : 0.f);
      for (int k = 0; k < 3; ++k) eik[k] = (gn > 0.f) ? ls * w_eik * sg * o.grad[k] / gn * invM : 0.f;
      for (int i = 0; i < 3; ++i) {
        const float a0 = o.A[i][0], a1 = o.A[i][1], a2 = o.A[i][2];
        const float an = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
        l_gd += an;
        const float sc_ = (an > 0.f) ? ls * w_dyn * invM / (3.f * an) : 0.f;
        gdef_bar[i][0] = a0 * sc_; gdef_bar[i][1] = a1 * sc_; gdef_bar[i][2] = a2 * sc_;
      }
      const float c = wo[3];
      l_c = fabsf(c);
      corr_bar = ls * w_dyn * invM * ((c > 0.f) ? 1.f : (c < 0.f ? -1.f : 0.f));
      const float sd = o.sdf - o.vp;
      l_sd = fabsf(sd);
      sdef_bar = ls * w_dyn * invM * ((sd > 0.f) ? 1.f : (sd < 0.f ? -1.f : 0.f));
    }
    for (int k = 0; k < 3; ++k) {
      gg[k] = ((g_gradient ? g_gradient[m * 3 + k] : 0.f) + eik[k]) + cos_bar * v[k];
      vb[k] = cos_bar * o.grad[k];
    }
    // ---- grad = A gq + Jc
    float Abar[3][3], gq_bar[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        Abar[i][j] = gg[i] * o.gq[j] + (PRIORS ? gdef_bar[i][j] : (g_grad_deform ? g_grad_deform[m * 9 + i * 3 + j] : 0.f));
    for (int j = 0; j < 3; ++j) gq_bar[j] = o.A[0][j] * gg[0] + o.A[1][j] * gg[1] + o.A[2][j] * gg[2];
    float sd_up = PRIORS ? sdef_bar : (g_sdf_deform ? g_sdf_deform[m] : 0.f);
    float sdf_tot = sdf_bar + sd_up;
    float c_bar = sdf_tot + (PRIORS ? corr_bar : (g_correction ? g_correction[m] : 0.f));
    float vq_bar = sdf_tot, vp_bar = -sd_up;
    // ---- trilinear backward at q (value + gradient outputs) and p (value only)
    float gu[3], hu[3];
    tri_grad(tq, Gq, gu, hu);
    float gqb_u[3] = {gq_bar[0] * scl[0], gq_bar[1] * scl[1], gq_bar[2] * scl[2]};  // upstream wrt d/du
    float q_bar[3];
    q_bar[0] = (vq_bar * gu[0] + hu[0] * gqb_u[1] + hu[1] * gqb_u[2]) * scl[0];
    q_bar[1] = (vq_bar * gu[1] + hu[0] * gqb_u[0] + hu[2] * gqb_u[2]) * scl[1];
    q_bar[2] = (vq_bar * gu[2] + hu[1] * gqb_u[0] + hu[2] * gqb_u[1]) * scl[2];
    float gpu[3], hpu[3];
    tri_grad(tp, Gp, gpu, hpu);
    float pb[3];
    for (int k = 0; k < 3; ++k) pb[k] = vp_bar * gpu[k] * scl[k] + q_bar[k];
    // ---- alpha / beta gradients through the corner mapping
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float sx = (c & 4) ? 1.f : -1.f, sy = (c & 2) ? 1.f : -1.f, sz = (c & 1) ? 1.f : -1.f;
      float wx = (c & 4) ? tq.w1[0] : tq.w0[0], wy = (c & 2) ? tq.w1[1] : tq.w0[1], wz = (c & 1) ? tq.w1[2] : tq.w0[2];
      float coef = vq_bar * (wx * wy * wz) + gqb_u[0] * (sx * wy * wz) + gqb_u[1] * (wx * sy * wz) + gqb_u[2] * (wx * wy * sz);
      float sg = Gq[c] / mp.A + 0.5f;
      ga_sum += coef * mp.dA * (sg - 0.5f);
      gb_sum += coef * mp.A * sg * (1.f - sg) * Sq[c] * mp.dB;
      float wxp = (c & 4) ? tp.w1[0] : tp.w0[0], wyp = (c & 2) ? tp.w1[1] : tp.w0[1], wzp = (c & 1) ? tp.w1[2] : tp.w0[2];
      float coefp = vp_bar * (wxp * wyp * wzp);
      float sgp = Gp[c] / mp.A + 0.5f;
      ga_sum += coefp * mp.dA * (sgp - 0.5f);
      gb_sum += coefp * mp.A * sgp * (1.f - sgp) * Sp[c] * mp.dB;
    }
    // ---- outputs
    float wg[16];
    wg[0] = q_bar[0]; wg[1] = q_bar[1]; wg[2] = q_bar[2]; wg[3] = c_bar;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) wg[(1 + i) * 4 + j] = Abar[i][j]; wg[(1 + i) * 4 + 3] = gg[i]; }
    float4* o4 = reinterpret_cast<float4*>(warp_out_grad + (size_t)m * 16);
    for (int i = 0; i < 4; ++i) o4[i] = make_float4(wg[i * 4], wg[i * 4 + 1], wg[i * 4 + 2], wg[i * 4 + 3]);
    for (int k = 0; k < 3; ++k) {
      if (accumulate) { pts_grad[m * 3 + k] += pb[k]; if (vgrad_s) vgrad_s[m * 3 + k] += vb[k]; }
      else { pts_grad[m * 3 + k] = pb[k]; if (vgrad_s) vgrad_s[m * 3 + k] = vb[k]; }
    }
  }
  // block reduction of the two scalar gradients, one atomic pair per block
  ga_sum = pp_wave_sum(ga_sum);
  gb_sum = pp_wave_sum(gb_sum);
  int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[0][wid] = ga_sum; red[1][wid] = gb_sum; }
  if (PRIORS) {
    l_eik = pp_wave_sum(l_eik); l_gd = pp_wave_sum(l_gd); l_c = pp_wave_sum(l_c); l_sd = pp_wave_sum(l_sd);
    if (lane == 0) { red[2][wid] = l_eik; red[3][wid] = l_gd; red[4][wid] = l_c; red[5][wid] = l_sd; }
  }
  __syncthreads();
  // the sums of a work-group: wavefront partials added in order; ONE atomic per value and work-group - all work-groups finish
  // together and the six addresses serve ~10 ns per atomic, so the kernel runs with GEO_BWD_THREADS = 512 (108 live work-groups
  // at the train step's 55 k samples: 24.4 -> 18.1 us; 14.1 us with no atomics at all; 1024 threads would spill)
  if (threadIdx.x < 6) {
    float s = 0.f;
    const int nw = blockDim.x >> 6;
    for (int w = 0; w < nw; ++w) s += red[threadIdx.x][w];
    const int k = threadIdx.x;
    if (k < 2) {
      // part != nullptr (ordered flush, pp_ordered.h): the work-group's sums go to its row, every work-group writes one
      if (part) part[blockIdx.x * ORD_GEO_ROW + k] = s;
      else if (sdf_ab_grad && s != 0.f) atomicAdd(&sdf_ab_grad[k], s);
    } else if (PRIORS && loss_out && blockIdx.x * blockDim.x < M) {
      atomicAdd(&loss_out[k], k == 3 ? s * invM / 3.f : s * invM);
    }
  }
}

extern "C" int pp_geometry_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                               const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                               const int32_t* count, int32_t capacity, float inv_s, float* alpha, float* gradient,
                               float* sdf_final, float* sdf_deform, float* grad_deform, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && warp_out && viewdirs && ray_id && count && alpha && gradient,
             "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  hipLaunchKernelGGL(k_geometry_fwd, dim3(pp_div_up(capacity, 256)), dim3(256), 0, pp_stream(stream), pp_scene_dev(sc),
                     sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient,
                     sdf_final, sdf_deform, grad_deform);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_geometry_bwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                               const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                               const int32_t* count, int32_t capacity, float inv_s, const float* g_alpha,
                               const float* g_gradient, const float* g_sdf_final, const float* g_sdf_deform,
                               const float* g_grad_deform, const float* g_correction, int32_t accumulate,
                               float* warp_out_grad, float* pts_grad, float* viewdir_grad_s, float* sdf_ab_grad,
                               void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && warp_out && viewdirs && ray_id && count && warp_out_grad && pts_grad,
             "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  hipLaunchKernelGGL(k_geometry_bwd<false>, dim3(pp_div_up(capacity, GEO_BWD_THREADS)), dim3(GEO_BWD_THREADS), 0, pp_stream(stream), pp_scene_dev(sc),
                     sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                     g_sdf_final, g_sdf_deform, g_grad_deform, g_correction, accumulate, warp_out_grad, pts_grad,
                     viewdir_grad_s, sdf_ab_grad, 0.f, 0.f, 0.f, (float*)nullptr, (const float*)nullptr, (float*)nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_geometry_bwd_priors(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                      const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                                      const int32_t* count, int32_t capacity, float inv_s, const float* g_alpha,
                                      const float* g_gradient, float w_eikonal, float w_deform, float loss_scale,
                                      int32_t accumulate, float* warp_out_grad, float* pts_grad, float* viewdir_grad_s,
                                      float* sdf_ab_grad, float* loss_out, const float* batch_norm, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && warp_out && viewdirs && ray_id && count && warp_out_grad && pts_grad,
             "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  hipLaunchKernelGGL(k_geometry_bwd<true>, dim3(pp_div_up(capacity, GEO_BWD_THREADS)), dim3(GEO_BWD_THREADS), 0, pp_stream(stream), pp_scene_dev(sc),
                     sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                     nullptr, nullptr, nullptr, nullptr, accumulate, warp_out_grad, pts_grad, viewdir_grad_s, sdf_ab_grad,
                     w_eikonal, w_deform, loss_scale, loss_out, batch_norm, (float*)nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// pp_geometry_bwd_priors with sdf_ab_grad added up in a fixed order: every work-group writes its two sums to its row of the
// context's ordered-flush workspace, one small reduction adds the rows (pp_ordered.h).  Everything else is the same kernel.
extern "C" int pp_geometry_bwd_priors_ordered(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                              const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                                              const int32_t* count, int32_t capacity, float inv_s, const float* g_alpha,
                                              const float* g_gradient, float w_eikonal, float w_deform, float loss_scale,
                                              int32_t accumulate, float* warp_out_grad, float* pts_grad, float* viewdir_grad_s,
                                              float* sdf_ab_grad, float* loss_out, const float* batch_norm, void* ctx, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && warp_out && viewdirs && ray_id && count && warp_out_grad && pts_grad && sdf_ab_grad,
             "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  const PPContext* c = static_cast<const PPContext*>(ctx);
  PP_REQUIRE(c && c->ord, "no ordered-flush workspace attached to the context (pp_ordered_attach)");
  PP_REQUIRE(capacity <= c->ord_cap, "the attached ordered-flush workspace is too small for this capacity");
  float* part = c->ord + pp_ord_layout(c->ord_wgs, c->ord_cap, c->ord_rays).geo;
  const int grid = pp_div_up(capacity, GEO_BWD_THREADS);
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_geometry_bwd<true>, dim3(grid), dim3(GEO_BWD_THREADS), 0, st, pp_scene_dev(sc),
                     sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                     nullptr, nullptr, nullptr, nullptr, accumulate, warp_out_grad, pts_grad, viewdir_grad_s, sdf_ab_grad,
                     w_eikonal, w_deform, loss_scale, loss_out, batch_norm, part);
  const OrdSegs segs{1, {2, 0, 0, 0}, {0, 0, 0, 0}};
  pp_launch_ordered_flush(part, ORD_GEO_ROW, grid, nullptr, 0, 1, segs, sdf_ab_grad, st);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// pp_geometry_fwd and pp_color_feat_fwd (k0_dim = 12, pos_pe = 5, view_pe = 1 only) in one launch: k_geometry_color_fwd
extern "C" int pp_geometry_color_feat_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                          const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                                          const int32_t* count, int32_t capacity, float inv_s, float* alpha, float* gradient,
                                          float* sdf_final, float* sdf_deform, float* grad_deform, const float* k0_cl,
                                          const float* pe_w, float* feat, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && warp_out && viewdirs && ray_id && count && alpha && gradient && k0_cl && pe_w && feat,
             "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE(sc->k0_dim == 12 && sc->pos_pe == 5 && sc->view_pe == 1, "the split feature row needs k0_dim = 12, pos_pe = 5, view_pe = 1");
  hipLaunchKernelGGL(k_geometry_color_fwd, dim3(2 * pp_div_up(capacity, 256)), dim3(256), 0, pp_stream(stream), pp_scene_dev(sc),
                     sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient, sdf_final,
                     sdf_deform, grad_deform, k0_cl, pe_w, feat);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
