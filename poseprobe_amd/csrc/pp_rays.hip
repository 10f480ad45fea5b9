// Pose algebra, index-first ray generation, dense / variable-length samplers with ray-major compaction.
// Reference behaviour restated (not translated) from: lib/camera.py:76-99,127-188; lib/recon_scene.py:62-74;
// lib/voxurf_coarse.py:1339-1368,1402-1407,697-719,936-945,661-695; lib/cuda/render_utils_kernel.cu:12-242.
#include "pp_common.h"
#include "pp_ordered.h"
#include "pp_ray_bwd.h"
#include "pp_pose_body.h"

__global__ void k_pose_fwd(const float* __restrict__ se3, const float* __restrict__ w2c_init,
                           const int32_t* __restrict__ refine_mask, int n_views, float* __restrict__ w2c,
                           float* __restrict__ c2w, float* __restrict__ jac) {
  pose_fwd_elem(blockIdx.x * blockDim.x + threadIdx.x, se3, w2c_init, refine_mask, n_views, w2c, c2w, jac);
}

__global__ void k_pose_bwd(const float* __restrict__ jac, const float* __restrict__ c2w_grad, int n_views,
                           float* __restrict__ se3_grad) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_views * 6) return;
  se3_grad[t] = pose_bwd_elem<false>(jac, c2w_grad, t);
}

extern "C" int pp_pose_fwd(const float* se3, const float* w2c_init, const int32_t* refine_mask, int32_t n_views,
                           float* w2c, float* c2w, float* jac, void* stream) {
  PP_REQUIRE(se3 && w2c_init && w2c && c2w && jac && n_views > 0, "null pointer or n_views<=0");
  hipLaunchKernelGGL(k_pose_fwd, dim3(pp_div_up(n_views * 6, 64)), dim3(64), 0, pp_stream(stream), se3, w2c_init,
                     refine_mask, n_views, w2c, c2w, jac);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
extern "C" int pp_pose_bwd(const float* jac, const float* c2w_grad, int32_t n_views, float* se3_grad, void* stream) {
  PP_REQUIRE(jac && c2w_grad && se3_grad && n_views > 0, "null pointer or n_views<=0");
  hipLaunchKernelGGL(k_pose_bwd, dim3(pp_div_up(n_views * 6, 64)), dim3(64), 0, pp_stream(stream), jac, c2w_grad,
                     n_views, se3_grad);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------
// ray generation for selected pixels
// ------------------------------------------------------------------------------------------------

__global__ void k_raygen_fwd(const int32_t* __restrict__ ray_idx, int n_rays, const float* __restrict__ c2w,
                             const float* __restrict__ intr, int H, int W, int inverse_y, int normalize,
                             const float* __restrict__ images, const float* __restrict__ masks,
                             float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ viewdirs,
                             float* __restrict__ target, float* __restrict__ mask_px) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays) return;
  int idx = ray_idx[r], view;
  float dirs[3];
  pixel_dir(idx, H, W, intr, inverse_y, view, dirs);
  const float* P = c2w + view * 12;
  float d[3];
  for (int k = 0; k < 3; ++k)  // torch.sum over the last dim of 3 products: (p0+p1)+p2
    d[k] = pp_add(pp_add(pp_mul(dirs[0], P[k * 4 + 0]), pp_mul(dirs[1], P[k * 4 + 1])), pp_mul(dirs[2], P[k * 4 + 2]));
  float nrm = pp_norm3(d[0], d[1], d[2]);
  for (int k = 0; k < 3; ++k) {
    float vd = pp_div(d[k], nrm);
    rays_o[r * 3 + k] = P[k * 4 + 3];
    rays_d[r * 3 + k] = normalize ? vd : d[k];
    viewdirs[r * 3 + k] = vd;
  }
  if (target) for (int k = 0; k < 3; ++k) target[r * 3 + k] = images[(size_t)idx * 3 + k];
  if (mask_px) mask_px[r] = masks[idx];
}

extern "C" int pp_raygen_select_fwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                                    const float* intr, int32_t n_views, int32_t H, int32_t W, int32_t inverse_y,
                                    int32_t normalize, const float* images, const float* masks, float* rays_o,
                                    float* rays_d, float* viewdirs, float* target, float* mask_px, void* stream) {
  (void)sc; (void)n_views;
  PP_REQUIRE(ray_idx && c2w && intr && rays_o && rays_d && viewdirs && n_rays > 0, "null pointer or n_rays<=0");
  PP_REQUIRE((!target || images) && (!mask_px || masks), "target/mask requested without images/masks");
  hipLaunchKernelGGL(k_raygen_fwd, dim3(pp_div_up(n_rays, 256)), dim3(256), 0, pp_stream(stream), ray_idx, n_rays,
                     c2w, intr, H, W, inverse_y, normalize, images, masks, rays_o, rays_d, viewdirs, target, mask_px);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------
// dense sampler (sample_ray_ori) : one wavefront per ray, lanes = sample slots
// ------------------------------------------------------------------------------------------------
struct RaySlab {
  float o[3], d[3], t_min, t_max, nrm;
  bool miss;
};

__device__ __forceinline__ RaySlab ray_slab(const SceneDev& sc, const float* __restrict__ rays_o,
                                            const float* __restrict__ rays_d, int r) {
  RaySlab s;
  float lo = -INFINITY, hi = INFINITY;
  for (int k = 0; k < 3; ++k) {
    s.o[k] = rays_o[r * 3 + k];
    s.d[k] = rays_d[r * 3 + k];
    float vec = (s.d[k] == 0.f) ? 1e-6f : s.d[k];
    float a = pp_div(pp_sub(sc.mx[k], s.o[k]), vec);
    float b = pp_div(pp_sub(sc.mn[k], s.o[k]), vec);
    lo = fmaxf(lo, fminf(a, b));
    hi = fminf(hi, fmaxf(a, b));
  }
  s.t_min = fminf(fmaxf(lo, sc.near_), sc.far_);
  s.t_max = fminf(fmaxf(hi, sc.near_), sc.far_);
  s.miss = (s.t_max <= s.t_min);
  s.nrm = pp_norm3(s.d[0], s.d[1], s.d[2]);
  return s;
}

// in-bbox test of sample slot k; returns step and point
__device__ __forceinline__ bool dense_sample(const SceneDev& sc, const RaySlab& s, float stepdist, float jit, int k,
                                             float& step, float p[3]) {
  float rng = pp_add((float)k, jit);
  step = pp_mul(stepdist, rng);
  float interpx = pp_add(s.t_min, pp_div(step, s.nrm));
  bool out = s.miss;
  for (int c = 0; c < 3; ++c) {
    p[c] = pp_add(s.o[c], pp_mul(s.d[c], interpx));
    out |= (sc.mn[c] > p[c]) | (p[c] > sc.mx[c]);
  }
  return !out;
}

__global__ __launch_bounds__(256) void k_sample_count(SceneDev sc, const float* __restrict__ rays_o,
                                                      const float* __restrict__ rays_d,
                                                      const float* __restrict__ jitter, int n_rays,
                                                      float* __restrict__ t_min, float* __restrict__ t_max,
                                                      int32_t* __restrict__ counts) {
  int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  RaySlab s = ray_slab(sc, rays_o, rays_d, r);
  float stepdist = pp_mul(sc.stepsize, sc.voxel);
  float jit = jitter ? jitter[r] : 0.f;
  int cnt = 0;
  for (int k0 = 0; k0 < sc.S; k0 += 64) {
    int k = k0 + lane;
    float step, p[3];
    bool keep = (k < sc.S) && dense_sample(sc, s, stepdist, jit, k, step, p);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) {
    counts[r] = cnt;
    t_min[r] = s.t_min;
    t_max[r] = s.t_max;
  }
}

// exclusive scan of counts[0..n) into start[0..n], every entry clamped to the capacity: start[n] = count_out[0] =
// min(total, capacity), so every per-ray range [start[r], start[r+1]) a later kernel walks lies inside the allocation (rays past
// the capacity become empty, the ray that straddles it is cut)
__global__ __launch_bounds__(1024) void k_exclusive_scan(const int32_t* __restrict__ counts, int n,
                                                         int32_t* __restrict__ start, int32_t* __restrict__ count_out,
                                                         int capacity) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    int i = base + tid;
    int v = (i < n) ? counts[i] : 0;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) { int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) wsum[wid] = x;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wid; ++w) woff += wsum[w];
    int carry = carry_s;
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

__global__ __launch_bounds__(256) void k_sample_fill(SceneDev sc, const float* __restrict__ rays_o,
                                                     const float* __restrict__ rays_d,
                                                     const float* __restrict__ jitter, int n_rays, int capacity,
                                                     const int32_t* __restrict__ ray_start, float* __restrict__ pts,
                                                     int32_t* __restrict__ ray_id, int32_t* __restrict__ step_k,
                                                     float* __restrict__ step_out, uint8_t* __restrict__ mask_keep) {
  int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  RaySlab s = ray_slab(sc, rays_o, rays_d, r);
  float stepdist = pp_mul(sc.stepsize, sc.voxel);
  float jit = jitter ? jitter[r] : 0.f;
  int base = ray_start[r];
  for (int k0 = 0; k0 < sc.S; k0 += 64) {
    int k = k0 + lane;
    float step, p[3];
    bool keep = (k < sc.S) && dense_sample(sc, s, stepdist, jit, k, step, p);
    unsigned long long bal = __ballot(keep);
    int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (mask_keep && k < sc.S) mask_keep[(size_t)r * sc.S + k] = keep ? 1 : 0;
    if (keep && pos < capacity) {
      pts[pos * 3 + 0] = p[0]; pts[pos * 3 + 1] = p[1]; pts[pos * 3 + 2] = p[2];
      ray_id[pos] = r;
      step_k[pos] = k;
      step_out[pos] = step;
    }
    base += __popcll(bal);
  }
}

extern "C" int pp_sample_dense(const pp_scene* sc, const float* rays_o, const float* rays_d, const float* jitter,
                               int32_t n_rays, int32_t capacity, float* t_min, float* t_max, int32_t* ray_start,
                               int32_t* count, float* pts, int32_t* ray_id, int32_t* step_k, float* step,
                               uint8_t* mask_keep, void* stream) {
  PP_REQUIRE(sc && rays_o && rays_d && t_min && t_max && ray_start && count && pts && ray_id && step_k && step,
             "null pointer");
  PP_REQUIRE(n_rays > 0 && capacity > 0, "n_rays/capacity must be positive");
  SceneDev d = pp_scene_dev(sc);
  hipStream_t st = pp_stream(stream);
  // per-ray counts are staged in ray_start[0..N) and scanned in place into a second region: use step_k as scratch
  // is not possible (written later only), so counts live in ray_id's first N entries when capacity >= n_rays.
  PP_REQUIRE(capacity >= n_rays, "capacity must be >= n_rays (scratch reuse)");
  int32_t* counts = ray_id;
  hipLaunchKernelGGL(k_sample_count, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, d, rays_o, rays_d, jitter, n_rays,
                     t_min, t_max, counts);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, st, counts, n_rays, ray_start, count, capacity);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sample_fill, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, d, rays_o, rays_d, jitter, n_rays,
                     capacity, ray_start, pts, ray_id, step_k, step, mask_keep);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------
// variable-length sampler (sample_pts_on_rays semantics, then Voxurf.sample_ray_cuda's python post-processing)
// ------------------------------------------------------------------------------------------------
struct VarRay {
  float start[3], dir[3], view[3], t_min, t_max;
  int n;
};

__device__ __forceinline__ VarRay var_ray(const SceneDev& sc, const float* __restrict__ rays_o,
                                          const float* __restrict__ rays_d, int r, float stepdist) {
  VarRay v;
  float o[3], d[3];
  float lo = -INFINITY, hi = INFINITY;
  for (int k = 0; k < 3; ++k) {
    o[k] = rays_o[r * 3 + k]; d[k] = rays_d[r * 3 + k];
    float vec = (d[k] == 0.f) ? 1e-6f : d[k];
    float a = pp_div(pp_sub(sc.mx[k], o[k]), vec), b = pp_div(pp_sub(sc.mn[k], o[k]), vec);
    lo = fmaxf(lo, fminf(a, b));
    hi = fminf(hi, fmaxf(a, b));
  }
  const float far = 1e9f;  // voxurf_coarse.py:673
  v.t_min = fmaxf(fminf(lo, far), sc.near_);
  v.t_max = fmaxf(fminf(hi, far), sc.near_);
  // kernel.cu:49-54 plain products, no contraction
  float rn = sqrtf(pp_add(pp_add(pp_mul(d[0], d[0]), pp_mul(d[1], d[1])), pp_mul(d[2], d[2])));
  float ns = ceilf(pp_div(pp_mul(pp_sub(v.t_max, v.t_min), rn), stepdist));
  v.n = (ns < 1.f || !(ns == ns)) ? 1 : (int)fminf(ns, 1.0e6f);
  float tn = pp_norm3(d[0], d[1], d[2]);  // torch-side rays_d.norm() (voxurf_coarse.py:682)
  for (int k = 0; k < 3; ++k) {
    v.start[k] = pp_add(o[k], pp_mul(d[k], v.t_min));
    v.dir[k] = pp_div(d[k], rn);
    v.view[k] = pp_div(d[k], tn);
  }
  return v;
}

__device__ __forceinline__ bool var_keep(const SceneDev& sc, const VarRay& v, float stepdist, int s) {
  float dist = pp_mul(stepdist, (float)s);
  bool out = false;
  for (int k = 0; k < 3; ++k) {
    float p = pp_add(v.start[k], pp_mul(v.dir[k], dist));
    out |= (sc.mn[k] > p) | (sc.mx[k] < p);
  }
  return !out;
}

__global__ __launch_bounds__(256) void k_var_count(SceneDev sc, const float* __restrict__ rays_o,
                                                   const float* __restrict__ rays_d, int n_rays,
                                                   float* __restrict__ t_min, float* __restrict__ t_max,
                                                   int32_t* __restrict__ n_steps, int32_t* __restrict__ counts) {
  int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  float stepdist = pp_mul(sc.stepsize, sc.voxel);
  VarRay v = var_ray(sc, rays_o, rays_d, r, stepdist);
  int cnt = 0;
  for (int s0 = 0; s0 < v.n; s0 += 64) {
    int s = s0 + lane;
    bool keep = (s < v.n) && var_keep(sc, v, stepdist, s);
    cnt += __popcll(__ballot(keep));
  }
  if (lane == 0) { counts[r] = cnt; n_steps[r] = v.n; t_min[r] = v.t_min; t_max[r] = v.t_max; }
}

__global__ __launch_bounds__(256) void k_var_fill(SceneDev sc, const float* __restrict__ rays_o,
                                                  const float* __restrict__ rays_d, int n_rays, int capacity,
                                                  const int32_t* __restrict__ ray_start, float* __restrict__ pts,
                                                  int32_t* __restrict__ ray_id, int32_t* __restrict__ step_id) {
  int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  float stepdist = pp_mul(sc.stepsize, sc.voxel);
  VarRay v = var_ray(sc, rays_o, rays_d, r, stepdist);
  int base = ray_start[r];
  for (int s0 = 0; s0 < v.n; s0 += 64) {
    int s = s0 + lane;
    bool keep = (s < v.n) && var_keep(sc, v, stepdist, s);
    unsigned long long bal = __ballot(keep);
    int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep && pos < capacity) {
      // rays_start[ray_id] + rays_view[ray_id] * step_id * stepdist   (voxurf_coarse.py:683)
      for (int k = 0; k < 3; ++k) pts[pos * 3 + k] = pp_add(v.start[k], pp_mul(pp_mul(v.view[k], (float)s), stepdist));
      ray_id[pos] = r;
      step_id[pos] = s;
    }
    base += __popcll(bal);
  }
}

extern "C" int pp_sample_var(const pp_scene* sc, const float* rays_o, const float* rays_d, int32_t n_rays,
                             int32_t capacity, float* t_min, float* t_max, int32_t* n_steps, int32_t* ray_start,
                             int32_t* count, float* pts, int32_t* ray_id, int32_t* step_id, void* stream) {
  PP_REQUIRE(sc && rays_o && rays_d && t_min && t_max && n_steps && ray_start && count && pts && ray_id && step_id,
             "null pointer");
  PP_REQUIRE(n_rays > 0 && capacity >= n_rays, "need n_rays>0 and capacity>=n_rays");
  SceneDev d = pp_scene_dev(sc);
  hipStream_t st = pp_stream(stream);
  int32_t* counts = ray_id;
  hipLaunchKernelGGL(k_var_count, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, d, rays_o, rays_d, n_rays, t_min, t_max,
                     n_steps, counts);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, st, counts, n_rays, ray_start, count, capacity);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_var_fill, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, st, d, rays_o, rays_d, n_rays, capacity,
                     ray_start, pts, ray_id, step_id);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------
// backward: samples -> rays -> c2w.  One wavefront per ray (body: pp_ray_bwd.h).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_raygen_bwd(
    SceneDev sc, const int32_t* __restrict__ ray_idx, int n_rays, const float* __restrict__ c2w,
    const float* __restrict__ intr, int n_views, int H, int W, int inverse_y, const float* __restrict__ rays_o,
    const float* __restrict__ rays_d, const float* __restrict__ t_min, const int32_t* __restrict__ ray_start,
    const float* __restrict__ pts_grad, const float* __restrict__ step, const float* __restrict__ vgrad_s,
    const float* __restrict__ g_o_in, const float* __restrict__ g_d_in, const float* __restrict__ g_v_in,
    const float* __restrict__ g_depth, float* __restrict__ g_o_out, float* __restrict__ g_d_out,
    float* __restrict__ g_v_out, float* __restrict__ c2w_grad, float* __restrict__ part) {
  extern __shared__ float s_c2w[];  // [n_views*12]
  raygen_bwd_body<false>(blockIdx.x, s_c2w, sc, ray_idx, n_rays, c2w, intr, n_views, H, W, inverse_y, rays_o, rays_d, t_min, ray_start,
                         pts_grad, step, vgrad_s, g_o_in, g_d_in, g_v_in, g_depth, g_o_out, g_d_out, g_v_out, c2w_grad, part);
}


// Ordered flush of k_raygen_bwd: one work-group per view.  Thread t adds the rows (one per ray) of rays t, t + 256, ... that belong
// to its view, in ascending order, into twelve sums; the 256 x 12 partial sums are then folded by a tree with fixed pairs
// (t += t + 128, t += t + 64, ...), so the order of every addition is a function of n_rays alone.  Overwrites c2w_grad.
__global__ __launch_bounds__(256) void k_raygen_c2w_reduce(const float* __restrict__ part, int n_rays, int n_views,
                                                           float* __restrict__ c2w_grad) {
  __shared__ float sums[256][13];              // 13: the twelve columns of consecutive threads fall into different banks
  const int view = blockIdx.x, t = threadIdx.x;
  float s[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) s[e] = 0.f;
  const float4* __restrict__ rows = reinterpret_cast<const float4*>(part);
  for (int r = t; r < n_rays; r += 256) {
    const float4 tail = rows[(size_t)r * (ORD_RAY_ROW / 4) + 3];                    // | view | pad
    if (__float_as_int(tail.x) != view) continue;
    const float4 a = rows[(size_t)r * (ORD_RAY_ROW / 4)], b = rows[(size_t)r * (ORD_RAY_ROW / 4) + 1],
                 c = rows[(size_t)r * (ORD_RAY_ROW / 4) + 2];
    s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    s[4] += b.x; s[5] += b.y; s[6] += b.z; s[7] += b.w;
    s[8] += c.x; s[9] += c.y; s[10] += c.z; s[11] += c.w;
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) sums[t][e] = s[e];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int e = 0; e < 12; ++e) sums[t][e] += sums[t + h][e];
    }
    __syncthreads();
  }
  if (t < 12) c2w_grad[view * 12 + t] = sums[0][t];
}

static int raygen_select_bwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w, const float* intr,
                             int32_t n_views, int32_t H, int32_t W, int32_t inverse_y, const float* rays_o, const float* rays_d,
                             const float* t_min, const int32_t* ray_start, const float* pts_grad, const float* step,
                             const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                             const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out, float* rays_d_grad_out,
                             float* viewdirs_grad_out, float* c2w_grad, float* part, void* stream);

extern "C" int pp_raygen_select_bwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                                    const float* intr, int32_t n_views, int32_t H, int32_t W, int32_t inverse_y,
                                    const float* rays_o, const float* rays_d, const float* t_min,
                                    const int32_t* ray_start, const float* pts_grad, const float* step,
                                    const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                                    const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out,
                                    float* rays_d_grad_out, float* viewdirs_grad_out, float* c2w_grad, void* stream) {
  PP_REQUIRE(sc && rays_o && rays_d && t_min && ray_start && pts_grad && step, "null pointer");
  PP_REQUIRE(!c2w_grad || (ray_idx && c2w && intr && n_views > 0), "c2w_grad requested without camera data");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  return raygen_select_bwd(sc, ray_idx, n_rays, c2w, intr, n_views, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step,
                           viewdir_grad_s, rays_o_grad, rays_d_grad, viewdirs_grad, depth_grad, rays_o_grad_out, rays_d_grad_out,
                           viewdirs_grad_out, c2w_grad, nullptr, stream);
}

// pp_raygen_select_bwd with c2w_grad added up in ray order (required here) through the context's ordered-flush workspace
extern "C" int pp_raygen_select_bwd_ordered(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                                            const float* intr, int32_t n_views, int32_t H, int32_t W, int32_t inverse_y,
                                            const float* rays_o, const float* rays_d, const float* t_min,
                                            const int32_t* ray_start, const float* pts_grad, const float* step,
                                            const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                                            const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out,
                                            float* rays_d_grad_out, float* viewdirs_grad_out, float* c2w_grad, void* ctx,
                                            void* stream) {
  PP_REQUIRE(sc && rays_o && rays_d && t_min && ray_start && pts_grad && step && c2w_grad, "null pointer");
  PP_REQUIRE(ray_idx && c2w && intr && n_views > 0, "c2w_grad requested without camera data");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  const PPContext* c = static_cast<const PPContext*>(ctx);
  PP_REQUIRE(c && c->ord, "no ordered-flush workspace attached to the context (pp_ordered_attach)");
  PP_REQUIRE(n_rays <= c->ord_rays, "the attached ordered-flush workspace is too small for this ray count");
  return raygen_select_bwd(sc, ray_idx, n_rays, c2w, intr, n_views, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step,
                           viewdir_grad_s, rays_o_grad, rays_d_grad, viewdirs_grad, depth_grad, rays_o_grad_out, rays_d_grad_out,
                           viewdirs_grad_out, c2w_grad, c->ord + pp_ord_layout(c->ord_wgs, c->ord_cap, c->ord_rays).ray, stream);
}

static int raygen_select_bwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w, const float* intr,
                             int32_t n_views, int32_t H, int32_t W, int32_t inverse_y, const float* rays_o, const float* rays_d,
                             const float* t_min, const int32_t* ray_start, const float* pts_grad, const float* step,
                             const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                             const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out, float* rays_d_grad_out,
                             float* viewdirs_grad_out, float* c2w_grad, float* part, void* stream) {
  SceneDev d = pp_scene_dev(sc);
  hipStream_t st = pp_stream(stream);
  if (c2w_grad) {
    if (hipMemsetAsync(c2w_grad, 0, sizeof(float) * 12 * n_views, st) != hipSuccess) {
      pp_set_error("pp_raygen_select_bwd: memset failed");
      return PP_ERR_LAUNCH;
    }
  }
  int nv = n_views > 0 ? n_views : 1;
  hipLaunchKernelGGL(k_raygen_bwd, dim3(pp_div_up(n_rays, 4)), dim3(256), sizeof(float) * 12 * nv, st, d, ray_idx,
                     n_rays, c2w, intr, nv, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step,
                     viewdir_grad_s, rays_o_grad, rays_d_grad, viewdirs_grad, depth_grad, rays_o_grad_out,
                     rays_d_grad_out, viewdirs_grad_out, c2w_grad, part);
  if (part) hipLaunchKernelGGL(k_raygen_c2w_reduce, dim3(nv), dim3(256), 0, st, part, n_rays, nv, c2w_grad);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
