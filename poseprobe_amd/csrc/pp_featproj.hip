// Surface-projection feature loss of the object branch on a second small ray batch.
//
//   reference: lib/recon_scene.py:371-439 (get_project_feature_loss), :610-619 (its place in the loss); lib/camera.py:251-253
//   (world2cam); lib/common.py:76-109 (get_tensor_values: grid_sample, bilinear, align_corners, zero padding), :450-465
//   (project_to_cam_real), :468-492 (project_to_cam); torch.nn.functional.cosine_similarity (eps = 1e-8: both norms are clamped
//   from below by eps OUTSIDE the graph, so the norm's own derivative a / |a| passes unmasked; 0 at the zero vector).
//
// Three launches after the reprojection (k_featproj_reproject) and the two renders:
//   k_featproj_geom  one work-group: the per-row flag (geometry only) and n_valid, counted in a fixed order;
//   k_featproj_rows  one wavefront per row, lanes across channels: the eight taps of a layer are eight contiguous runs of C floats
//                    (16 bytes per lane where C % 4 == 0); one pass gives the dot product, the two squared norms and the eight
//                    sums the positional derivatives need (they are linear in the taps), reduced over the 64 lanes by a butterfly;
//   k_featproj_fold  one work-group: the sums over rows (cos per layer, the two views' w2c gradients) in a fixed order.
// No atomics anywhere: the same inputs give the same bits.
#include "pp_common.h"

#define FPJ_T 256
#define FPJ_MAX_LAYERS 4
#define FPJ_MAX_C 512
#define FPJ_EPS 1e-8f

struct FpjLayers {
  int n;
  const float* feat[FPJ_MAX_LAYERS];            // [n_views, h, w, C] each
  int C[FPJ_MAX_LAYERS], h[FPJ_MAX_LAYERS], w[FPJ_MAX_LAYERS];
  int vec[FPJ_MAX_LAYERS];                       // C % 4 == 0 and a 16-byte aligned base: float4 loads
};

struct FpjArgs {
  int n_rows, capacity, n_views, vi, vj, H, W;
  const float *o_a, *d_a, *tmin_a, *acc_a, *o_b, *d_b, *tmin_b, *acc_b, *intr, *w2c;
  float nl, voxel;
};

// camera-frame point of view v with the near-plane replacement (recon_scene.py:415-419); true: replaced (a constant: no gradient)
__device__ __forceinline__ bool fpj_cam(const float* __restrict__ w2c, int v, const float p[3], float nl, float q[3]) {
  const float* W = w2c + v * 12;
  for (int a = 0; a < 3; ++a) q[a] = W[a * 4] * p[0] + W[a * 4 + 1] * p[1] + W[a * 4 + 2] * p[2] + W[a * 4 + 3];
  const bool behind = q[2] < nl;
  if (behind) q[0] = q[1] = q[2] = nl;
  return behind;
}

__device__ __forceinline__ void fpj_surface(const float* __restrict__ o, const float* __restrict__ d,
                                            const float* __restrict__ t_min, const float* __restrict__ acc, int r, float p[3],
                                            float* depth, bool* hit) {
  const float a = acc[r];
  *depth = t_min[r] + a;
  *hit = a > 0.f;
  for (int k = 0; k < 3; ++k) p[k] = o[r * 3 + k] + d[r * 3 + k] * *depth;
}

// everything of one row that the flag and the gradients share
struct FpjRow {
  float p[3], d[3], depth;
  float qi[3], qj[3];
  bool behind_i, behind_j, valid;
  float xi, yi, xj, yj;                          // normalised image coordinates (project_to_cam)
};

__device__ __forceinline__ void fpj_norm_xy(const float* __restrict__ intr, int v, const float q[3], int H, int W, float* x, float* y) {
  const float* K = intr + v * 4;
  const float u = (K[0] * q[0] + K[2] * q[2]) / q[2];
  const float vv = (K[1] * q[1] + K[3] * q[2]) / q[2];
  *x = 2.f * u / (float)(W - 1) - 1.f;
  *y = 2.f * vv / (float)(H - 1) - 1.f;
}

__device__ __forceinline__ void fpj_row(const FpjArgs& A, int r, FpjRow& w) {
  bool hit_a, hit_b;
  float p_ref[3], depth_b;
  fpj_surface(A.o_a, A.d_a, A.tmin_a, A.acc_a, r, w.p, &w.depth, &hit_a);
  fpj_surface(A.o_b, A.d_b, A.tmin_b, A.acc_b, r, p_ref, &depth_b, &hit_b);
  for (int k = 0; k < 3; ++k) w.d[k] = A.d_a[r * 3 + k];
  const float dx = w.p[0] - p_ref[0], dy = w.p[1] - p_ref[1], dz = w.p[2] - p_ref[2];
  const bool close = sqrtf(dx * dx + dy * dy + dz * dz) < A.voxel * 2.f;
  w.behind_i = fpj_cam(A.w2c, A.vi, w.p, A.nl, w.qi);
  w.behind_j = fpj_cam(A.w2c, A.vj, w.p, A.nl, w.qj);
  fpj_norm_xy(A.intr, A.vi, w.qi, A.H, A.W, &w.xi, &w.yi);
  fpj_norm_xy(A.intr, A.vj, w.qj, A.H, A.W, &w.xj, &w.yj);
  const bool inside = fmaxf(fabsf(w.xi), fabsf(w.yi)) <= 1.f && fmaxf(fabsf(w.xj), fabsf(w.yj)) <= 1.f;
  w.valid = close && hit_a && hit_b && inside;
}

// ---------------------------------------------------------------------------------------------------------------------------
// step 2: surface point of query A into view vj -> the pixel query B shoots through; one thread per row
__global__ __launch_bounds__(FPJ_T) void k_featproj_reproject(int n_rows, int capacity, int vj, const float* __restrict__ o,
                                                              const float* __restrict__ d, const float* __restrict__ t_min,
                                                              const float* __restrict__ acc, const float* __restrict__ intr,
                                                              const float* __restrict__ w2c, float nl, int32_t* __restrict__ own_ref,
                                                              float* __restrict__ pix_ref) {
  const int r = blockIdx.x * FPJ_T + threadIdx.x;
  if (r >= capacity) return;
  if (r >= n_rows) {
    // not a row: view -1 is none - pp_reproj_rays gives it a ray that misses the box
    own_ref[r] = -1;
    pix_ref[2 * r] = pix_ref[2 * r + 1] = 0.f;
    return;
  }
  float p[3], q[3], depth;
  bool hit;
  fpj_surface(o, d, t_min, acc, r, p, &depth, &hit);
  fpj_cam(w2c, vj, p, nl, q);
  const float* K = intr + vj * 4;
  own_ref[r] = vj;
  pix_ref[2 * r] = (K[0] * q[0] + K[2] * q[2]) / q[2];
  pix_ref[2 * r + 1] = (K[1] * q[1] + K[3] * q[2]) / q[2];
}

extern "C" int pp_featproj_reproject(int32_t n_rows, int32_t capacity, int32_t view_j, const float* rays_o, const float* rays_d,
                                     const float* t_min, const float* acc, const float* intr, const float* w2c, int32_t n_views,
                                     float nl, int32_t* own_ref, float* pix_ref, void* stream) {
  PP_REQUIRE(rays_o && rays_d && t_min && acc && intr && w2c && own_ref && pix_ref, "null pointer");
  PP_REQUIRE(n_rows > 0 && n_rows <= capacity && n_views > 0, "need 0 < n_rows <= capacity and n_views > 0");
  PP_REQUIRE(view_j >= 0 && view_j < n_views, "view_j is no view");
  PP_REQUIRE(nl > 0.f, "the near plane must lie in front of the camera (nl > 0): the pixel is a quotient by max(q_z, nl)");
  hipLaunchKernelGGL(k_featproj_reproject, dim3(pp_div_up(capacity, FPJ_T)), dim3(FPJ_T), 0, pp_stream(stream), n_rows, capacity,
                     view_j, rays_o, rays_d, t_min, acc, intr, w2c, nl, own_ref, pix_ref);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// fixed-order tree over the FPJ_T partials of each of n rows of red[n][FPJ_T]; red[k][0] holds the sums afterwards
__device__ void fpj_tree(float (*red)[FPJ_T], int n) {
  __syncthreads();
  for (int o = FPJ_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int k = 0; k < n; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
}

__global__ __launch_bounds__(FPJ_T) void k_featproj_geom(FpjArgs A, uint8_t* __restrict__ valid, float* __restrict__ terms) {
  __shared__ float red[1][FPJ_T];
  const int tid = threadIdx.x;
  float part = 0.f;
  for (int r = tid; r < A.capacity; r += FPJ_T) {
    bool v = false;
    if (r < A.n_rows) {
      FpjRow w;
      fpj_row(A, r, w);
      v = w.valid;
    }
    valid[r] = v ? 1 : 0;
    part += v ? 1.f : 0.f;
  }
  red[0][tid] = part;
  fpj_tree(red, 1);
  if (tid == 0) terms[1] = red[0][0];
}

// One view's share of one layer: the four taps around (x, y) of feat[v] for this lane's channels, accumulated into
//   val[c] (the sample), dx[c], dy[c] (its derivatives by the continuous texel position; out-of-range taps are zeros, as
//   grid_sample's backward treats them)
struct FpjTaps {
  int off[4];                                    // element offset of the tap's run, or -1: outside the map
  float wgt[4], tx, ty;
};

__device__ __forceinline__ void fpj_taps(float x, float y, int v, int C, int h, int w, FpjTaps& t) {
  // grid_sample, align_corners: ((x + 1) / 2) (w - 1)
  const float ix = (x + 1.f) * 0.5f * (float)(w - 1), iy = (y + 1.f) * 0.5f * (float)(h - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  t.tx = ix - fx;
  t.ty = iy - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  t.wgt[0] = (1.f - t.tx) * (1.f - t.ty); t.wgt[1] = t.tx * (1.f - t.ty); t.wgt[2] = (1.f - t.tx) * t.ty; t.wgt[3] = t.tx * t.ty;
  for (int k = 0; k < 4; ++k) {
    const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
    const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
    t.off[k] = in ? ((v * h + yy) * w + xx) * C : -1;
  }
}

template <int N>
struct FpjVec { float v[N]; };

template <int N>
__device__ __forceinline__ FpjVec<N> fpj_load(const float* __restrict__ feat, int off, int c) {
  FpjVec<N> out;
  if (off < 0) {
    for (int k = 0; k < N; ++k) out.v[k] = 0.f;
  } else if (N == 4) {
    const float4 q = *reinterpret_cast<const float4*>(feat + off + c);
    out.v[0] = q.x; out.v[1] = q.y; out.v[2] = q.z; out.v[3] = q.w;
  } else {
    out.v[0] = feat[off + c];
  }
  return out;
}

// the eleven sums of one layer over this lane's channels: [0] a.b [1] a.a [2] b.b [3] b.da/dx [4] a.da/dx [5] b.da/dy [6] a.da/dy
// [7] a.db/dx [8] b.db/dx [9] a.db/dy [10] b.db/dy
template <int N>
__device__ __forceinline__ void fpj_channels(const float* __restrict__ feat, int C, const FpjTaps& ti, const FpjTaps& tj, int lane,
                                             float s[11]) {
  for (int c = lane * N; c < C; c += PP_WAVE * N) {
    FpjVec<N> a[4], b[4];
    for (int k = 0; k < 4; ++k) { a[k] = fpj_load<N>(feat, ti.off[k], c); b[k] = fpj_load<N>(feat, tj.off[k], c); }
    for (int e = 0; e < N; ++e) {
      const float va = ti.wgt[0] * a[0].v[e] + ti.wgt[1] * a[1].v[e] + ti.wgt[2] * a[2].v[e] + ti.wgt[3] * a[3].v[e];
      const float vb = tj.wgt[0] * b[0].v[e] + tj.wgt[1] * b[1].v[e] + tj.wgt[2] * b[2].v[e] + tj.wgt[3] * b[3].v[e];
      const float dax = (a[1].v[e] - a[0].v[e]) * (1.f - ti.ty) + (a[3].v[e] - a[2].v[e]) * ti.ty;
      const float day = (a[2].v[e] - a[0].v[e]) * (1.f - ti.tx) + (a[3].v[e] - a[1].v[e]) * ti.tx;
      const float dbx = (b[1].v[e] - b[0].v[e]) * (1.f - tj.ty) + (b[3].v[e] - b[2].v[e]) * tj.ty;
      const float dby = (b[2].v[e] - b[0].v[e]) * (1.f - tj.tx) + (b[3].v[e] - b[1].v[e]) * tj.tx;
      s[0] += va * vb; s[1] += va * va; s[2] += vb * vb;
      s[3] += vb * dax; s[4] += va * dax; s[5] += vb * day; s[6] += va * day;
      s[7] += va * dbx; s[8] += vb * dbx; s[9] += va * dby; s[10] += vb * dby;
    }
  }
}

// gradient on the camera-frame point from the gradient on the normalised image coordinates
__device__ __forceinline__ void fpj_cam_bwd(const float* __restrict__ intr, int v, const float q[3], bool behind, int H, int W, float gx,
                                            float gy, float gq[3]) {
  gq[0] = gq[1] = gq[2] = 0.f;
  if (behind) return;
  const float* K = intr + v * 4;
  const float gu = gx * 2.f / (float)(W - 1), gv = gy * 2.f / (float)(H - 1);
  const float iz = 1.f / q[2];
  // (u, v) = (fx q_x / q_z + cx, fy q_y / q_z + cy): the principal point drops out of d / d q_z
  gq[0] = K[0] * gu * iz;
  gq[1] = K[1] * gv * iz;
  gq[2] = -(K[0] * gu * q[0] + K[1] * gv * q[1]) * iz * iz;
}

__global__ __launch_bounds__(FPJ_T) void k_featproj_rows(FpjArgs A, FpjLayers Ls, float weight, float scale,
                                                         const uint8_t* __restrict__ valid, const float* __restrict__ terms,
                                                         float* __restrict__ cosv, float* __restrict__ g_q, float* __restrict__ g_depth,
                                                         float* __restrict__ g_o, float* __restrict__ g_d) {
  const int lane = threadIdx.x & (PP_WAVE - 1);
  const int r = blockIdx.x * (FPJ_T / PP_WAVE) + (threadIdx.x >> 6);
  if (r >= A.capacity) return;
  const float n_valid = terms[1];
  const bool live = r < A.n_rows && valid[r] != 0 && n_valid > 0.f;
  if (!live) {
    // rows that are none, rows the geometry rejects, and every row of a batch without a valid one: zeros
    if (lane < Ls.n) cosv[lane * A.capacity + r] = 0.f;
    if (lane < 6) g_q[r * 6 + lane] = 0.f;
    if (lane < 3) g_o[r * 3 + lane] = g_d[r * 3 + lane] = 0.f;
    if (lane == 0) g_depth[r] = 0.f;
    return;
  }
  FpjRow w;
  fpj_row(A, r, w);
  const float G = -scale * weight / n_valid;              // d (scale weight L) / d cos_r of every layer
  float gxi = 0.f, gyi = 0.f, gxj = 0.f, gyj = 0.f;
  for (int l = 0; l < Ls.n; ++l) {
    const int C = Ls.C[l], h = Ls.h[l], wd = Ls.w[l];
    FpjTaps ti, tj;
    fpj_taps(w.xi, w.yi, A.vi, C, h, wd, ti);
    fpj_taps(w.xj, w.yj, A.vj, C, h, wd, tj);
    float s[11];
    for (int k = 0; k < 11; ++k) s[k] = 0.f;
    if (Ls.vec[l]) fpj_channels<4>(Ls.feat[l], C, ti, tj, lane, s);
    else fpj_channels<1>(Ls.feat[l], C, ti, tj, lane, s);
    for (int k = 0; k < 11; ++k) s[k] = pp_wave_sum(s[k]);
    const float na = sqrtf(s[1]), nb = sqrtf(s[2]);
    const float ca = fmaxf(na, FPJ_EPS), cb = fmaxf(nb, FPJ_EPS);
    const float inv = 1.f / (ca * cb);
    const float c = s[0] * inv;
    // d cos / d a = b / (ca cb) - (a.b) / (ca^2 cb) a / |a|  (the norm's derivative, 0 at the zero vector); alike for b
    const float ka = na > 0.f ? s[0] / (ca * ca * cb * na) : 0.f;
    const float kb = nb > 0.f ? s[0] / (cb * cb * ca * nb) : 0.f;
    const float sx = 0.5f * (float)(wd - 1), sy = 0.5f * (float)(h - 1);   // texel position by normalised coordinate
    gxi += G * (s[3] * inv - ka * s[4]) * sx;
    gyi += G * (s[5] * inv - ka * s[6]) * sy;
    gxj += G * (s[7] * inv - kb * s[8]) * sx;
    gyj += G * (s[9] * inv - kb * s[10]) * sy;
    if (lane == 0) cosv[l * A.capacity + r] = c;
  }
  if (lane != 0) return;
  float gqi[3], gqj[3], gp[3];
  fpj_cam_bwd(A.intr, A.vi, w.qi, w.behind_i, A.H, A.W, gxi, gyi, gqi);
  fpj_cam_bwd(A.intr, A.vj, w.qj, w.behind_j, A.H, A.W, gxj, gyj, gqj);
  const float* Wi = A.w2c + A.vi * 12;
  const float* Wj = A.w2c + A.vj * 12;
  float gdep = 0.f;
  for (int b = 0; b < 3; ++b) {
    gp[b] = Wi[b] * gqi[0] + Wi[4 + b] * gqi[1] + Wi[8 + b] * gqi[2] + Wj[b] * gqj[0] + Wj[4 + b] * gqj[1] + Wj[8 + b] * gqj[2];
    gdep += gp[b] * w.d[b];
  }
  for (int b = 0; b < 3; ++b) {
    g_q[r * 6 + b] = gqi[b];
    g_q[r * 6 + 3 + b] = gqj[b];
    g_o[r * 3 + b] = gp[b];
    g_d[r * 3 + b] = w.depth * gp[b];
  }
  g_depth[r] = gdep;
}

// sums over rows: cos per layer -> terms; g_q (x) [p, 1] -> the two views' w2c gradients; every other view's is zero
__global__ __launch_bounds__(FPJ_T) void k_featproj_fold(FpjArgs A, int n_layers, const uint8_t* __restrict__ valid,
                                                         const float* __restrict__ cosv, const float* __restrict__ g_q,
                                                         float* __restrict__ terms, float* __restrict__ g_w2c) {
  __shared__ float red[24 + FPJ_MAX_LAYERS][FPJ_T];
  const int tid = threadIdx.x;
  float part[24 + FPJ_MAX_LAYERS];
  for (int k = 0; k < 24 + FPJ_MAX_LAYERS; ++k) part[k] = 0.f;
  const float n_valid = terms[1];
  if (n_valid > 0.f) {
    for (int r = tid; r < A.n_rows; r += FPJ_T) {
      if (!valid[r]) continue;
      float p[3], depth;
      bool hit;
      fpj_surface(A.o_a, A.d_a, A.tmin_a, A.acc_a, r, p, &depth, &hit);
      for (int v = 0; v < 2; ++v)
        for (int a = 0; a < 3; ++a) {
          const float g = g_q[r * 6 + v * 3 + a];
          for (int b = 0; b < 3; ++b) part[v * 12 + a * 4 + b] += g * p[b];
          part[v * 12 + a * 4 + 3] += g;
        }
      for (int l = 0; l < FPJ_MAX_LAYERS; ++l)
        if (l < n_layers) part[24 + l] += cosv[l * A.capacity + r];
    }
  }
  for (int k = 0; k < 24 + FPJ_MAX_LAYERS; ++k) red[k][tid] = part[k];
  fpj_tree(red, 24 + FPJ_MAX_LAYERS);
  for (int i = tid; i < A.n_views * 12; i += FPJ_T) {
    const int v = i / 12, k = i - v * 12;
    float g = 0.f;
    if (v == A.vi) g += red[k][0];
    if (v == A.vj) g += red[12 + k][0];
    g_w2c[i] = g;
  }
  if (tid == 0) {
    float loss = 0.f;
    for (int l = 0; l < FPJ_MAX_LAYERS; ++l) {
      const float sc = l < n_layers ? red[24 + l][0] : 0.f;
      terms[2 + l] = sc;
      if (l < n_layers && n_valid > 0.f) loss += 1.f - sc / n_valid;
    }
    terms[0] = loss;
  }
}

extern "C" int pp_featproj_loss(int32_t n_rows, int32_t capacity, int32_t view_i, int32_t view_j, const float* rays_o,
                                const float* rays_d, const float* t_min, const float* acc, const float* ref_rays_o,
                                const float* ref_rays_d, const float* ref_t_min, const float* ref_acc, const float* intr,
                                const float* w2c, int32_t n_views, float nl, float voxel_size, int32_t H, int32_t W,
                                int32_t n_layers, const float* feat0, const float* feat1, const float* feat2, const float* feat3,
                                const int32_t* layer_dims, float weight, float scale, float* terms, uint8_t* valid, float* cosv,
                                float* g_q, float* g_depth, float* g_o, float* g_d, float* g_w2c, void* stream) {
  PP_REQUIRE(rays_o && rays_d && t_min && acc && ref_rays_o && ref_rays_d && ref_t_min && ref_acc && intr && w2c, "null pointer");
  PP_REQUIRE(terms && valid && cosv && g_q && g_depth && g_o && g_d && g_w2c && layer_dims, "null pointer");
  PP_REQUIRE(n_rows > 0 && n_rows <= capacity && capacity < (1 << 24) && n_views > 0, "need 0 < n_rows <= capacity < 2^24 and n_views > 0");
  PP_REQUIRE(view_i >= 0 && view_i < n_views && view_j >= 0 && view_j < n_views, "view_i / view_j is no view");
  PP_REQUIRE(H >= 2 && W >= 2, "need H, W >= 2");
  PP_REQUIRE(n_layers >= 1 && n_layers <= FPJ_MAX_LAYERS, "need 1 <= n_layers <= 4");
  const float* feats[FPJ_MAX_LAYERS] = {feat0, feat1, feat2, feat3};
  FpjLayers Ls;
  Ls.n = n_layers;
  for (int l = 0; l < FPJ_MAX_LAYERS; ++l) {
    Ls.feat[l] = nullptr; Ls.C[l] = Ls.h[l] = Ls.w[l] = Ls.vec[l] = 0;
    if (l >= n_layers) continue;
    const int C = layer_dims[3 * l], h = layer_dims[3 * l + 1], w = layer_dims[3 * l + 2];
    PP_REQUIRE(feats[l], "null feature layer");
    PP_REQUIRE(C >= 1 && C <= FPJ_MAX_C && h >= 2 && w >= 2, "need 1 <= C <= 512 and h, w >= 2 in every layer");
    PP_REQUIRE((long long)n_views * h * w * C < (1ll << 31), "a feature layer holds 2^31 elements or more");
    Ls.feat[l] = feats[l]; Ls.C[l] = C; Ls.h[l] = h; Ls.w[l] = w;
    Ls.vec[l] = (C % 4 == 0 && reinterpret_cast<uintptr_t>(feats[l]) % 16 == 0) ? 1 : 0;
  }
  FpjArgs A;
  A.n_rows = n_rows; A.capacity = capacity; A.n_views = n_views; A.vi = view_i; A.vj = view_j; A.H = H; A.W = W;
  A.o_a = rays_o; A.d_a = rays_d; A.tmin_a = t_min; A.acc_a = acc;
  A.o_b = ref_rays_o; A.d_b = ref_rays_d; A.tmin_b = ref_t_min; A.acc_b = ref_acc;
  A.intr = intr; A.w2c = w2c; A.nl = nl; A.voxel = voxel_size;
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_featproj_geom, dim3(1), dim3(FPJ_T), 0, st, A, valid, terms);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_featproj_rows, dim3(pp_div_up(capacity, FPJ_T / PP_WAVE)), dim3(FPJ_T), 0, st, A, Ls, weight, scale, valid,
                     terms, cosv, g_q, g_depth, g_o, g_d);
  PP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_featproj_fold, dim3(1), dim3(FPJ_T), 0, st, A, n_layers, valid, cosv, g_q, terms, g_w2c);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
