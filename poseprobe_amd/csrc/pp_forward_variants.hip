// The two branches of Voxurf.forward / Voxurf.inference beside the default one:
//   * plain-template geometry (use_deform=False, lib/voxurf_coarse.py:986-989 with neus_sdf_gradient :458-467): no warp net; the
//     mapped grid G = softplus10(alpha) (sigmoid(softplus10(beta) sdf) - 0.5) is sampled with F.grid_sample semantics
//     (align_corners=True, border padding) and so is the 3-channel grid of its central differences.  One thread per sample gathers
//     the 8 corners and their 24 axis neighbours from the RAW sdf grid, maps them in registers and forms the differences there:
//     neither G nor the difference grid exists in memory.
//   * weight-threshold compaction (fast_color_thres > 0, :996-1003 / :1144-1151): one wavefront per ray keeps the samples whose
//     weight of the first composite exceeds the threshold (ballot + prefix count, as the dense sampler compacts).
#include "pp_common.h"
#include "pp_plain_body.h"

namespace {

constexpr int PLAIN_THREADS = 256;

__global__ __launch_bounds__(PLAIN_THREADS) void k_geometry_plain_fwd(
    SceneDev sc, const float* __restrict__ grid, const float* __restrict__ sdf_ab, const float* __restrict__ pts,
    const float* __restrict__ viewdirs, const int32_t* __restrict__ ray_id, const int32_t* __restrict__ count, int capacity,
    float inv_s, float* __restrict__ alpha, float* __restrict__ gradient, float* __restrict__ sdf_final) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int M = min(count[0], capacity);
  if (m >= M) return;
  const float A = pp_softplus10(sdf_ab[0]), B = pp_softplus10(sdf_ab[1]);
  const float p[3] = {pts[m * 3], pts[m * 3 + 1], pts[m * 3 + 2]};
  const int r = ray_id[m];
  const float v[3] = {viewdirs[r * 3], viewdirs[r * 3 + 1], viewdirs[r * 3 + 2]};
  PlainCell t;
  plain_setup(sc, p, t);
  float S[4][8], G[4][8];
  plain_gather(sc, grid, t, S);
  PlainFwd o;
  plain_forward(sc, t, A, B, S, v, inv_s, G, o);
  alpha[m] = fminf(fmaxf(o.a_un, 0.f), 1.f);
#pragma unroll
  for (int k = 0; k < 3; ++k) gradient[m * 3 + k] = o.grad[k];
  if (sdf_final) sdf_final[m] = o.sdf;
}

__global__ __launch_bounds__(PLAIN_THREADS) void k_geometry_plain_bwd(
    SceneDev sc, const float* __restrict__ grid, const float* __restrict__ sdf_ab, const float* __restrict__ pts,
    const float* __restrict__ viewdirs, const int32_t* __restrict__ ray_id, const int32_t* __restrict__ count, int capacity,
    float inv_s, const float* __restrict__ g_alpha, const float* __restrict__ g_gradient, const float* __restrict__ g_sdf_final,
    int accumulate, float* __restrict__ pts_grad, float* __restrict__ vgrad_s, float* __restrict__ sdf_ab_grad) {
  __shared__ float red[2][PLAIN_THREADS / 64];
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int M = min(count[0], capacity);
  float ga_sum = 0.f, gb_sum = 0.f;
  if (m < M) {
    const float A = pp_softplus10(sdf_ab[0]), B = pp_softplus10(sdf_ab[1]);
    const float dA = pp_dsoftplus10(sdf_ab[0]), dB = pp_dsoftplus10(sdf_ab[1]);
    const float p[3] = {pts[m * 3], pts[m * 3 + 1], pts[m * 3 + 2]};
    const int r = ray_id[m];
    const float v[3] = {viewdirs[r * 3], viewdirs[r * 3 + 1], viewdirs[r * 3 + 2]};
    PlainCell t;
    plain_setup(sc, p, t);
    float S[4][8], G[4][8];
    plain_gather(sc, grid, t, S);
    PlainFwd o;
    plain_forward(sc, t, A, B, S, v, inv_s, G, o);
    const float dist = pp_mul(sc.stepsize, sc.voxel);
    // ---- alpha backward (clip passes the gradient on the closed interval, as torch.clamp)
    float ga = g_alpha ? g_alpha[m] : 0.f;
    if (!(o.a_un >= 0.f && o.a_un <= 1.f)) ga = 0.f;
    const float n_bar = ga / o.den;
    const float d_bar = -ga * o.num / (o.den * o.den);
    const float pc_bar = n_bar + d_bar, nc_bar = -n_bar;
    const float prv_bar = pc_bar * o.pc * (1.f - o.pc) * inv_s;
    const float nxt_bar = nc_bar * o.nc * (1.f - o.nc) * inv_s;
    const float sdf_bar = prv_bar + nxt_bar + (g_sdf_final ? g_sdf_final[m] : 0.f);
    const float ic_bar = (nxt_bar - prv_bar) * (dist * 0.5f);
    const float cos_bar = (o.cosv < 0.f) ? ic_bar : 0.f;
    float gg[3], vb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gg[k] = (g_gradient ? g_gradient[m * 3 + k] : 0.f) + cos_bar * v[k];
      vb[k] = cos_bar * o.grad[k];
    }
    // ---- both trilinear lookups: d/d(coordinate) through the corner weights, d/d(mapped value) into coef
    const float h = 0.5f / sc.voxel;            // d(central difference) / d(its upper neighbour)
    float coef[4][8];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int c = 0; c < 8; ++c) coef[g][c] = 0.f;
    float du[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int dx = (c >> 2) & 1, dy = (c >> 1) & 1, dz = c & 1;
      const float wx = t.w[0][dx], wy = t.w[1][dy], wz = t.w[2][dz];
      const float w = (wx * wy) * wz;
      const float val_bar = sdf_bar * G[0][c] + ((gg[0] * o.D[0][c] + gg[1] * o.D[1][c]) + gg[2] * o.D[2][c]);
      du[0] += (dx ? val_bar : -val_bar) * (wy * wz);
      du[1] += (dy ? val_bar : -val_bar) * (wx * wz);
      du[2] += (dz ? val_bar : -val_bar) * (wx * wy);
      coef[0][c] += sdf_bar * w;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int d = (c & axis_bit(a)) ? 1 : 0;
        if (t.cd[a][d]) {
          const float b_ = (gg[a] * w) * h;
          coef[1 + a][c] += d ? b_ : -b_;
          coef[0][c ^ axis_bit(a)] += d ? -b_ : b_;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float sg = G[g][c] / A + 0.5f;
        ga_sum += coef[g][c] * dA * (sg - 0.5f);
        gb_sum += coef[g][c] * A * sg * (1.f - sg) * S[g][c] * dB;
      }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float scl = (float)(sc.sz[k] - 1) / (sc.mx[k] - sc.mn[k]);
      const float pb = du[k] * scl * t.gm[k];
      if (accumulate) { pts_grad[m * 3 + k] += pb; if (vgrad_s) vgrad_s[m * 3 + k] += vb[k]; }
      else { pts_grad[m * 3 + k] = pb; if (vgrad_s) vgrad_s[m * 3 + k] = vb[k]; }
    }
  }
  // the two scalar gradients: wavefront sums, added per work-group in order, ONE atomic per value and work-group (k_geometry_bwd's flush)
  ga_sum = pp_wave_sum(ga_sum);
  gb_sum = pp_wave_sum(gb_sum);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[0][wid] = ga_sum; red[1][wid] = gb_sum; }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
    const int nw = blockDim.x >> 6;
    for (int w = 0; w < nw; ++w) s += red[threadIdx.x][w];
    if (sdf_ab_grad && s != 0.f) atomicAdd(&sdf_ab_grad[threadIdx.x], s);
  }
}

// ------------------------------------------------------------------------------------------------ weight-threshold compaction
// one wavefront per ray, four rays per work-group.  `counts` is new_start[0 .. n_rays): scanned in place by k_keep_scan.
__global__ __launch_bounds__(256) void k_keep_count(const float* __restrict__ weights, const int32_t* __restrict__ ray_start,
                                                    int n_rays, int capacity, float thres, int32_t* __restrict__ counts) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int b = min(max(ray_start[r], 0), capacity), e = min(max(ray_start[r + 1], b), capacity);
  int cnt = 0;
  for (int c0 = b; c0 < e; c0 += 64) {
    const int i = c0 + lane;
    const bool keep = (i < e) && (weights[i] > thres);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) counts[r] = cnt;
}

// exclusive scan of start[0 .. n) IN PLACE (every thread reads its own entries before it overwrites them); start[n] = count_out[0] =
// the total, every entry clamped to the capacity
__global__ __launch_bounds__(1024) void k_keep_scan(int32_t* start, int n, int32_t* __restrict__ count_out, int capacity) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int v = (i < n) ? start[i] : 0;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) { int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wsum[w];
    const int carry = carry_s;
    if (i < n) start[i] = min(carry + woff + x - v, capacity);
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + x;
    __syncthreads();
  }
  if (tid == 0) {
    const int total = carry_s < capacity ? carry_s : capacity;
    start[n] = total;
    count_out[0] = total;
  }
}

__global__ __launch_bounds__(256) void k_keep_fill(const float* __restrict__ weights, const int32_t* __restrict__ ray_start, int n_rays,
                                                   int capacity, float thres, const int32_t* __restrict__ new_start,
                                                   const float* __restrict__ pts, const int32_t* __restrict__ ray_id,
                                                   const float* __restrict__ step, const float* __restrict__ alpha,
                                                   const float* __restrict__ gradient, int32_t* __restrict__ kept_idx,
                                                   float* __restrict__ pts_k, int32_t* __restrict__ ray_id_k,
                                                   float* __restrict__ step_k, float* __restrict__ alpha_k,
                                                   float* __restrict__ gradient_k) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int b = min(max(ray_start[r], 0), capacity), e = min(max(ray_start[r + 1], b), capacity);
  int base = new_start[r];
  for (int c0 = b; c0 < e; c0 += 64) {
    const int i = c0 + lane;
    const bool keep = (i < e) && (weights[i] > thres);
    const unsigned long long bal = __ballot(keep);
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep && pos >= 0 && pos < capacity) {
      kept_idx[pos] = i;
      ray_id_k[pos] = ray_id[i];
      step_k[pos] = step[i];
      alpha_k[pos] = alpha[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        pts_k[pos * 3 + k] = pts[i * 3 + k];
        gradient_k[pos * 3 + k] = gradient[i * 3 + k];
      }
    }
    base += __popcll(bal);
  }
}

// backward of the gather: row kept_idx[j] of every full-length buffer receives row j of its kept twin (one-to-one: plain stores);
// the entry point zeroes the full-length buffers first
__global__ __launch_bounds__(256) void k_keep_scatter(const int32_t* __restrict__ kept_idx, const int32_t* __restrict__ kept_count,
                                                      int capacity, const float* __restrict__ g_alpha_k,
                                                      const float* __restrict__ g_gradient_k, const float* __restrict__ g_pts_k,
                                                      const float* __restrict__ g_view_k, float* __restrict__ g_alpha,
                                                      float* __restrict__ g_gradient, float* __restrict__ g_pts,
                                                      float* __restrict__ g_view) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(kept_count[0], capacity)) return;
  const int m = kept_idx[j];
  if (m < 0 || m >= capacity) return;
  if (g_alpha) g_alpha[m] = g_alpha_k[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (g_gradient) g_gradient[m * 3 + k] = g_gradient_k[j * 3 + k];
    if (g_pts) g_pts[m * 3 + k] = g_pts_k[j * 3 + k];
    if (g_view) g_view[m * 3 + k] = g_view_k[j * 3 + k];
  }
}

}  // namespace

extern "C" int pp_geometry_plain_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                     const float* viewdirs, const int32_t* ray_id, const int32_t* count, int32_t capacity,
                                     float inv_s, float* alpha, float* gradient, float* sdf_final, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && viewdirs && ray_id && count && alpha && gradient, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE(sc->size[0] >= 2 && sc->size[1] >= 2 && sc->size[2] >= 2, "the template needs two nodes along every axis");
  hipLaunchKernelGGL(k_geometry_plain_fwd, dim3(pp_div_up(capacity, PLAIN_THREADS)), dim3(PLAIN_THREADS), 0, pp_stream(stream),
                     pp_scene_dev(sc), sdf_grid, sdf_ab, pts, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient, sdf_final);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_geometry_plain_bwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                     const float* viewdirs, const int32_t* ray_id, const int32_t* count, int32_t capacity,
                                     float inv_s, const float* g_alpha, const float* g_gradient, const float* g_sdf_final,
                                     int32_t accumulate, float* pts_grad, float* viewdir_grad_s, float* sdf_ab_grad, void* stream) {
  PP_REQUIRE(sc && sdf_grid && sdf_ab && pts && viewdirs && ray_id && count && pts_grad, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE(sc->size[0] >= 2 && sc->size[1] >= 2 && sc->size[2] >= 2, "the template needs two nodes along every axis");
  hipLaunchKernelGGL(k_geometry_plain_bwd, dim3(pp_div_up(capacity, PLAIN_THREADS)), dim3(PLAIN_THREADS), 0, pp_stream(stream),
                     pp_scene_dev(sc), sdf_grid, sdf_ab, pts, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                     g_sdf_final, accumulate, pts_grad, viewdir_grad_s, sdf_ab_grad);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_keep_compact(const float* weights, const int32_t* ray_start, int32_t n_rays, int32_t capacity, float thres,
                               const float* pts, const int32_t* ray_id, const float* step, const float* alpha,
                               const float* gradient, int32_t* kept_idx, int32_t* kept_ray_start, int32_t* kept_count,
                               float* pts_k, int32_t* ray_id_k, float* step_k, float* alpha_k, float* gradient_k, void* stream) {
  PP_REQUIRE(weights && ray_start && pts && ray_id && step && alpha && gradient && kept_idx && kept_ray_start && kept_count && pts_k &&
                 ray_id_k && step_k && alpha_k && gradient_k,
             "null pointer");
  PP_REQUIRE(n_rays > 0 && capacity > 0, "n_rays/capacity must be positive");
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_keep_count, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, weights, ray_start, n_rays, capacity, thres,
                     kept_ray_start);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(1024), 0, st, kept_ray_start, n_rays, kept_count, capacity);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_keep_fill, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, weights, ray_start, n_rays, capacity, thres,
                     kept_ray_start, pts, ray_id, step, alpha, gradient, kept_idx, pts_k, ray_id_k, step_k, alpha_k, gradient_k);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_keep_scatter_bwd(const int32_t* kept_idx, const int32_t* kept_count, int32_t capacity, const float* g_alpha_k,
                                   const float* g_gradient_k, const float* g_pts_k, const float* g_view_k, float* g_alpha,
                                   float* g_gradient, float* g_pts, float* g_view, void* stream) {
  PP_REQUIRE(kept_idx && kept_count, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE((!g_alpha || g_alpha_k) && (!g_gradient || g_gradient_k) && (!g_pts || g_pts_k) && (!g_view || g_view_k),
             "a full-length gradient without its kept twin");
  hipStream_t st = pp_stream(stream);
  struct { float* p; size_t n; } full[4] = {{g_alpha, 1}, {g_gradient, 3}, {g_pts, 3}, {g_view, 3}};
  for (auto& f : full) {
    if (!f.p) continue;
    if (hipMemsetAsync(f.p, 0, f.n * (size_t)capacity * sizeof(float), st) != hipSuccess) {
      pp_set_error("%s: hipMemsetAsync failed", __func__);
      return PP_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(k_keep_scatter, dim3(pp_div_up(capacity, 256)), dim3(256), 0, st, kept_idx, kept_count, capacity, g_alpha_k,
                     g_gradient_k, g_pts_k, g_view_k, g_alpha, g_gradient, g_pts, g_view);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
