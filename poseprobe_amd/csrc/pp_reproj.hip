// Reprojection + near-surface pose terms of the object branch on a second small ray batch.
//
//   reference: lib/recon_scene.py:93-113 (get_ray_dir, mode 'no_center'), :313-319 (point_to_ray_distance), :321-369
//   (get_project_error); lib/camera.py:251-253 (world2cam); lib/common.py:450-465 (project_to_cam_real); lib/losses.py:77-103
//   (compute_diff_loss, 'huber'); lib/voxurf_coarse.py:701-705 (slab test), :697-719 (sample_ray_ori).
//
// The loss kernel is one work-group, the pose fold one work-group per view; both sum in a fixed order (strided per-thread
// partials, then a tree over the 256 partials), no atomics: the same inputs give the same bits, as pp_nerf_corres.hip.
#include "pp_common.h"

#define RPJ_T 256

__device__ __forceinline__ float rpj_norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, pp_mul(x, x)))); }

// camera-frame direction of a pixel (no half-pixel shift, inverse_y)
__device__ __forceinline__ void rpj_cam(const float* __restrict__ pix, const float* __restrict__ K, int r, float cam[3]) {
  cam[0] = pp_div(pp_sub(pix[2 * r], K[2]), K[0]);
  cam[1] = pp_div(pp_sub(pix[2 * r + 1], K[3]), K[1]);
  cam[2] = 1.f;
}

__global__ __launch_bounds__(RPJ_T) void k_reproj_rays(SceneDev sc, const int32_t* __restrict__ own, const float* __restrict__ pix,
                                                       int n_rows, int capacity, const float* __restrict__ intr,
                                                       const float* __restrict__ c2w, int n_views, float* __restrict__ rays_o,
                                                       float* __restrict__ rays_d, float* __restrict__ viewdirs) {
  const int r = blockIdx.x * RPJ_T + threadIdx.x;
  if (r >= capacity) return;
  const int v = r < n_rows ? own[r] : -1;
  float o[3], d[3];
  if (v >= 0 && v < n_views) {
    float cam[3];
    rpj_cam(pix, intr + v * 4, r, cam);
    const float* P = c2w + v * 12;
    for (int k = 0; k < 3; ++k) {
      d[k] = pp_add(pp_add(pp_mul(cam[0], P[k * 4 + 0]), pp_mul(cam[1], P[k * 4 + 1])), pp_mul(cam[2], P[k * 4 + 2]));
      o[k] = P[k * 4 + 3];
    }
    const float nrm = rpj_norm3(d[0], d[1], d[2]);
    for (int k = 0; k < 3; ++k) d[k] = pp_div(d[k], nrm);
  } else {
    // not a row: a ray that starts beyond the box's far corner and leaves it - the slab test gives t_max <= t_min, no sample
    for (int k = 0; k < 3; ++k) { o[k] = sc.mx[k] + 1.f; d[k] = k == 2 ? 1.f : 0.f; }
  }
  for (int k = 0; k < 3; ++k) { rays_o[r * 3 + k] = o[k]; rays_d[r * 3 + k] = d[k]; viewdirs[r * 3 + k] = d[k]; }
}

extern "C" int pp_reproj_rays(const pp_scene* sc, const int32_t* own, const float* pix, int32_t n_rows, int32_t capacity,
                              const float* intr, const float* c2w, int32_t n_views, float* rays_o, float* rays_d, float* viewdirs,
                              void* stream) {
  PP_REQUIRE(sc && own && pix && intr && c2w && rays_o && rays_d && viewdirs, "null pointer");
  PP_REQUIRE(n_rows > 0 && n_rows <= capacity && n_views > 0, "need 0 < n_rows <= capacity and n_views > 0");
  hipLaunchKernelGGL(k_reproj_rays, dim3(pp_div_up(capacity, RPJ_T)), dim3(RPJ_T), 0, pp_stream(stream), pp_scene_dev(sc), own, pix,
                     n_rows, capacity, intr, c2w, n_views, rays_o, rays_d, viewdirs);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// one thread per dense slot, the op order of the sampler (pp_rays.hip dense_sample)
__global__ __launch_bounds__(RPJ_T) void k_reproj_dense_pts(SceneDev sc, const float* __restrict__ rays_o,
                                                            const float* __restrict__ rays_d, const float* __restrict__ t_min,
                                                            const float* __restrict__ jitter, int n_rays, float* __restrict__ pts) {
  const int i = blockIdx.x * RPJ_T + threadIdx.x;
  if (i >= n_rays * sc.S) return;
  const int r = i / sc.S, k = i - r * sc.S;
  const float o[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
  const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
  const float nrm = rpj_norm3(d[0], d[1], d[2]);
  const float step = pp_mul(pp_mul(sc.stepsize, sc.voxel), pp_add((float)k, jitter ? jitter[r] : 0.f));
  const float interpx = pp_add(t_min[r], pp_div(step, nrm));
  for (int c = 0; c < 3; ++c) pts[(size_t)i * 3 + c] = pp_add(o[c], pp_mul(d[c], interpx));
}

extern "C" int pp_reproj_dense_pts(const pp_scene* sc, const float* rays_o, const float* rays_d, const float* t_min,
                                   const float* jitter, int32_t n_rays, float* pts, void* stream) {
  PP_REQUIRE(sc && rays_o && rays_d && t_min && pts, "null pointer");
  PP_REQUIRE(n_rays > 0 && sc->n_samples > 0 && (long long)n_rays * sc->n_samples < (1ll << 30), "bad sizes");
  hipLaunchKernelGGL(k_reproj_dense_pts, dim3(pp_div_up(n_rays * sc->n_samples, RPJ_T)), dim3(RPJ_T), 0, pp_stream(stream),
                     pp_scene_dev(sc), rays_o, rays_d, t_min, jitter, n_rays, pts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// fixed-order tree over the RPJ_T partials of each of n rows of red[n][RPJ_T]; red[k][0] holds the sums afterwards
__device__ void rpj_tree(float (*red)[RPJ_T], int n) {
  __syncthreads();
  for (int o = RPJ_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < n; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
}

struct RpjArgs {
  int render, n_rows, capacity, n_views, pixel_check;
  const int32_t* other;
  const float *match, *conf, *rays_o, *rays_d, *p, *t_min, *acc, *intr, *w2c;
  const uint8_t* hit;
  float centre[3], half_diag, nl, pixel_thre;
};

// everything of one row that the sums and the gradients share
struct RpjRow {
  float o[3], d[3], p[3], depth, c;
  float q[3], u, v, dx, dy, e;           // camera-frame point of the other view (after the near-plane replacement), pixel, error
  bool valid;
  float near;                            // max(dist - half_diag, 0) [c > 0]
  float s[3], t, dist;                   // centre - o, its projection on d, distance
};

__device__ __forceinline__ void rpj_row(const RpjArgs& A, int r, int vo, RpjRow& w) {
  for (int k = 0; k < 3; ++k) { w.o[k] = A.rays_o[r * 3 + k]; w.d[k] = A.rays_d[r * 3 + k]; }
  w.c = A.conf[r];
  bool hit;
  if (A.render) {
    const float acc = A.acc[r];
    w.depth = A.t_min[r] + acc;
    hit = acc > 0.f;
    for (int k = 0; k < 3; ++k) w.p[k] = w.o[k] + w.d[k] * w.depth;
  } else {
    w.depth = 0.f;
    hit = A.hit[r] != 0;
    for (int k = 0; k < 3; ++k) w.p[k] = A.p[r * 3 + k];
  }
  // near-surface term
  w.t = 0.f;
  for (int k = 0; k < 3; ++k) { w.s[k] = A.centre[k] - w.o[k]; w.t += w.s[k] * w.d[k]; }
  if (w.t < 0.f) {
    w.dist = sqrtf(w.s[0] * w.s[0] + w.s[1] * w.s[1] + w.s[2] * w.s[2]);
  } else {
    float n2 = 0.f;
    for (int k = 0; k < 3; ++k) { const float x = w.s[k] - w.t * w.d[k]; n2 += x * x; }
    w.dist = sqrtf(n2);
  }
  w.near = fmaxf(w.dist - A.half_diag, 0.f) * (w.c > 0.f ? 1.f : 0.f);
  // reprojection into the other view
  const float* W = A.w2c + vo * 12;
  const float* K = A.intr + vo * 4;
  for (int a = 0; a < 3; ++a) w.q[a] = W[a * 4] * w.p[0] + W[a * 4 + 1] * w.p[1] + W[a * 4 + 2] * w.p[2] + W[a * 4 + 3];
  const bool behind = w.q[2] < A.nl;
  if (behind) w.q[0] = w.q[1] = w.q[2] = A.nl;
  w.u = (K[0] * w.q[0] + K[2] * w.q[2]) / w.q[2];
  w.v = (K[1] * w.q[1] + K[3] * w.q[2]) / w.q[2];
  w.dx = w.u - A.match[2 * r];
  w.dy = w.v - A.match[2 * r + 1];
  w.e = sqrtf(w.dx * w.dx + w.dy * w.dy);
  w.valid = !behind && hit && (!A.pixel_check || w.e <= A.pixel_thre);
}

__device__ __forceinline__ float rpj_huber(float e) { return e < 1.f ? 0.5f * e * e : e - 0.5f; }

__global__ __launch_bounds__(RPJ_T) void k_reproj_loss(RpjArgs A, float w_near, float w_proj, float scale, float* __restrict__ terms,
                                                       float* __restrict__ g_p, float* __restrict__ g_depth,
                                                       float* __restrict__ g_o, float* __restrict__ g_d,
                                                       float* __restrict__ g_w2c) {
  __shared__ float red[12][RPJ_T];
  __shared__ float n_valid_s;
  const int tid = threadIdx.x;
  // ---- phase 1: the three sums
  float part[3] = {0.f, 0.f, 0.f};
  for (int r = tid; r < A.n_rows; r += RPJ_T) {
    const int vo = A.other[r];
    if (vo < 0 || vo >= A.n_views) continue;
    RpjRow w;
    rpj_row(A, r, vo, w);
    if (w.valid) { part[0] += 1.f; part[1] += w.c * rpj_huber(w.e); }
    part[2] += w.near;
  }
  for (int k = 0; k < 3; ++k) red[k][tid] = part[k];
  rpj_tree(red, 3);
  if (tid == 0) {
    n_valid_s = red[0][0];
    terms[0] = red[1][0] / (red[0][0] + 1e-6f);
    terms[1] = red[2][0];
    terms[2] = red[0][0];
  }
  __syncthreads();
  const float g_err = scale * w_proj / (n_valid_s + 1e-6f), g_near = scale * w_near;

  // ---- phase 2: per-row gradients, and per other view the direct gradient on its w2c
  for (int r = tid; r < A.capacity; r += RPJ_T) {            // rows that are none
    const int vo = r < A.n_rows ? A.other[r] : -1;
    if (vo >= 0 && vo < A.n_views) continue;
    for (int k = 0; k < 3; ++k) g_p[r * 3 + k] = g_o[r * 3 + k] = g_d[r * 3 + k] = 0.f;
    g_depth[r] = 0.f;
  }
  for (int view = 0; view < A.n_views; ++view) {
    float gs[12];
    for (int k = 0; k < 12; ++k) gs[k] = 0.f;
    int mine = 0;
    for (int r = tid; r < A.n_rows; r += RPJ_T) {
      if (A.other[r] != view) continue;
      mine = 1;
      RpjRow w;
      rpj_row(A, r, view, w);
      float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f};
      // near-surface term: clamp passes the gradient where dist - half >= 0 (torch), the norm's gradient is 0 at 0
      if (w.c > 0.f && w.dist - A.half_diag >= 0.f && w.dist > 0.f) {
        const float gn = g_near / w.dist;
        if (w.t < 0.f) {
          for (int k = 0; k < 3; ++k) go[k] = -gn * w.s[k];
        } else {
          float x[3], xd = 0.f;
          for (int k = 0; k < 3; ++k) { x[k] = gn * (w.s[k] - w.t * w.d[k]); xd += x[k] * w.d[k]; }
          for (int k = 0; k < 3; ++k) {
            go[k] = -(x[k] - xd * w.d[k]);
            gd[k] = -w.t * x[k] - xd * w.s[k];
          }
        }
      }
      if (w.valid && w.e > 0.f) {
        const float* W = A.w2c + view * 12;
        const float* K = A.intr + view * 4;
        const float G = g_err * w.c * fminf(w.e, 1.f) / w.e;
        const float gu = G * w.dx, gv = G * w.dy;
        const float iz = 1.f / w.q[2];
        // (u, v) = (fx q_x / q_z + cx, fy q_y / q_z + cy): the principal point drops out of d / d q_z
        const float gq[3] = {K[0] * gu * iz, K[1] * gv * iz, -(K[0] * gu * w.q[0] + K[1] * gv * w.q[1]) * iz * iz};
        for (int a = 0; a < 3; ++a) {
          for (int b = 0; b < 3; ++b) gs[a * 4 + b] += gq[a] * w.p[b];
          gs[a * 4 + 3] += gq[a];
        }
        for (int b = 0; b < 3; ++b) gp[b] = W[b] * gq[0] + W[4 + b] * gq[1] + W[8 + b] * gq[2];
      }
      float gdep = 0.f;
      if (A.render) {
        for (int k = 0; k < 3; ++k) { go[k] += gp[k]; gd[k] += w.depth * gp[k]; gdep += gp[k] * w.d[k]; }
      }
      for (int k = 0; k < 3; ++k) { g_p[r * 3 + k] = gp[k]; g_o[r * 3 + k] = go[k]; g_d[r * 3 + k] = gd[k]; }
      g_depth[r] = gdep;
    }
    // one barrier: the previous view's sums have been read, and a view no row projects into (most of them, with many views
    // and a few pairs per step) costs no tree
    if (!__syncthreads_or(mine)) {
      if (tid < 12) g_w2c[view * 12 + tid] = 0.f;
      continue;
    }
    for (int k = 0; k < 12; ++k) red[k][tid] = gs[k];
    rpj_tree(red, 12);
    if (tid < 12) g_w2c[view * 12 + tid] = red[tid][0];
  }
}

extern "C" int pp_reproj_loss(int32_t render, int32_t n_rows, int32_t capacity, const int32_t* other, const float* match,
                              const float* conf, const float* rays_o, const float* rays_d, const float* p, const uint8_t* hit,
                              const float* t_min, const float* acc, const float* intr, const float* w2c, int32_t n_views,
                              float centre_x, float centre_y, float centre_z, float half_diagonal, float nl,
                              int32_t pixel_check, float pixel_thre, float w_near, float w_proj, float scale, float* terms,
                              float* g_p, float* g_depth, float* g_o, float* g_d, float* g_w2c, void* stream) {
  PP_REQUIRE(other && match && conf && rays_o && rays_d && intr && w2c && terms && g_p && g_depth && g_o && g_d && g_w2c,
             "null pointer");
  PP_REQUIRE(render ? (t_min && acc) : (p && hit), "render = 1 needs t_min and acc, render = 0 needs p and hit");
  PP_REQUIRE(n_rows > 0 && n_rows <= capacity && n_views > 0, "need 0 < n_rows <= capacity and n_views > 0");
  RpjArgs A;
  A.render = render ? 1 : 0; A.n_rows = n_rows; A.capacity = capacity; A.n_views = n_views; A.pixel_check = pixel_check ? 1 : 0;
  A.other = other; A.match = match; A.conf = conf; A.rays_o = rays_o; A.rays_d = rays_d; A.p = p; A.t_min = t_min; A.acc = acc;
  A.intr = intr; A.w2c = w2c; A.hit = hit;
  A.centre[0] = centre_x; A.centre[1] = centre_y; A.centre[2] = centre_z;
  A.half_diag = half_diagonal; A.nl = nl; A.pixel_thre = pixel_thre;
  hipLaunchKernelGGL(k_reproj_loss, dim3(1), dim3(RPJ_T), 0, pp_stream(stream), A, w_near, w_proj, scale, terms, g_p, g_depth, g_o,
                     g_d, g_w2c);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// d t_min / d (o, d) of the slab test (amax / minimum / clamp with torch's tie handling), as k_raygen_bwd chains it
__device__ __forceinline__ void rpj_slab_bwd(const SceneDev& sc, const float o[3], const float d[3], float tmin_bar, float ob[3],
                                             float db[3]) {
  float ra[3], rb[3], lo[3], vec[3];
  float tm_raw = -INFINITY;
  for (int k = 0; k < 3; ++k) {
    vec[k] = (d[k] == 0.f) ? 1e-6f : d[k];
    ra[k] = (sc.mx[k] - o[k]) / vec[k];
    rb[k] = (sc.mn[k] - o[k]) / vec[k];
    lo[k] = fminf(ra[k], rb[k]);
    tm_raw = fmaxf(tm_raw, lo[k]);
  }
  if (!(tm_raw >= sc.near_ && tm_raw <= sc.far_) || tmin_bar == 0.f) return;
  int nmax = 0;
  for (int k = 0; k < 3; ++k) nmax += (lo[k] == tm_raw);
  for (int k = 0; k < 3; ++k) {
    if (lo[k] != tm_raw) continue;
    const float lb = tmin_bar / (float)nmax;
    const float wa = ra[k] < rb[k] ? 1.f : (ra[k] == rb[k] ? 0.5f : 0.f);
    const float rab = lb * wa, rbb = lb * (1.f - wa);
    ob[k] -= (rab + rbb) / vec[k];
    if (d[k] != 0.f) db[k] -= (rab * ra[k] + rbb * rb[k]) / vec[k];
  }
}

// work-group `view`: the rows whose own view it is, through d = normalize(R cam), o = t of c2w[view]
__global__ __launch_bounds__(RPJ_T) void k_reproj_pose_fold(SceneDev sc, const int32_t* __restrict__ own,
                                                            const float* __restrict__ pix, int n_rows,
                                                            const float* __restrict__ intr, const float* __restrict__ c2w,
                                                            const float* __restrict__ w2c, const float* __restrict__ rays_o,
                                                            const float* __restrict__ rays_d, const float* __restrict__ g_o,
                                                            const float* __restrict__ g_d, const float* __restrict__ g_v,
                                                            const float* __restrict__ g_t_min, const float* __restrict__ g_w2c,
                                                            float* __restrict__ g_c2w) {
  __shared__ float red[12][RPJ_T];
  const int view = blockIdx.x, tid = threadIdx.x;
  const float* P = c2w + view * 12;
  float part[12];
  for (int k = 0; k < 12; ++k) part[k] = 0.f;
  for (int r = tid; r < n_rows; r += RPJ_T) {
    if (own[r] != view) continue;
    float ob[3], db[3];
    for (int k = 0; k < 3; ++k) {
      ob[k] = g_o[r * 3 + k];
      db[k] = g_d[r * 3 + k] + (g_v ? g_v[r * 3 + k] : 0.f);
    }
    if (g_t_min) {
      const float o[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
      const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
      rpj_slab_bwd(sc, o, d, g_t_min[r], ob, db);
    }
    float cam[3], Du[3];
    rpj_cam(pix, intr + view * 4, r, cam);
    for (int k = 0; k < 3; ++k) Du[k] = cam[0] * P[k * 4 + 0] + cam[1] * P[k * 4 + 1] + cam[2] * P[k * 4 + 2];
    const float Dn = sqrtf(Du[0] * Du[0] + Du[1] * Du[1] + Du[2] * Du[2]);
    const float nh[3] = {Du[0] / Dn, Du[1] / Dn, Du[2] / Dn};
    const float dot = nh[0] * db[0] + nh[1] * db[1] + nh[2] * db[2];
    for (int k = 0; k < 3; ++k) {
      const float Db = (db[k] - nh[k] * dot) / Dn;
      for (int j = 0; j < 3; ++j) part[k * 4 + j] += Db * cam[j];
      part[k * 4 + 3] += ob[k];
    }
  }
  for (int k = 0; k < 12; ++k) red[k][tid] = part[k];
  rpj_tree(red, 12);
  if (tid < 12) {
    const int a = tid / 4, b = tid % 4;
    float g = red[tid][0];
    if (g_w2c) {
      // w2c = [R^T | -R^T t]: the algebra of k_nerf_pair_pose_bwd
      const float* Pw = w2c + view * 12;
      const float* gP = g_w2c + view * 12;
      if (b < 3) {
        const float c = -(Pw[a] * Pw[3] + Pw[4 + a] * Pw[7] + Pw[8 + a] * Pw[11]);      // camera centre = c2w[:, 3]
        g += gP[b * 4 + a] - c * gP[b * 4 + 3];
      } else {
        g += -(Pw[a] * gP[3] + Pw[4 + a] * gP[7] + Pw[8 + a] * gP[11]);
      }
    }
    g_c2w[view * 12 + tid] = g;
  }
}

extern "C" int pp_reproj_pose_fold(const pp_scene* sc, const int32_t* own, const float* pix, int32_t n_rows, const float* intr,
                                   const float* c2w, const float* w2c, int32_t n_views, const float* rays_o, const float* rays_d,
                                   const float* g_o, const float* g_d, const float* g_viewdirs, const float* g_t_min,
                                   const float* g_w2c, float* g_c2w, void* stream) {
  PP_REQUIRE(sc && own && pix && intr && c2w && g_o && g_d && g_c2w, "null pointer");
  PP_REQUIRE(!g_t_min || (rays_o && rays_d), "g_t_min needs rays_o and rays_d");
  PP_REQUIRE(!g_w2c || w2c, "g_w2c needs w2c");
  PP_REQUIRE(n_rows > 0 && n_views > 0, "bad sizes");
  hipLaunchKernelGGL(k_reproj_pose_fold, dim3(n_views), dim3(RPJ_T), 0, pp_stream(stream), pp_scene_dev(sc), own, pix, n_rows, intr,
                     c2w, w2c, rays_o, rays_d, g_o, g_d, g_viewdirs, g_t_min, g_w2c, g_c2w);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
