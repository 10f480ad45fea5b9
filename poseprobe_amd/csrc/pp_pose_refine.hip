// Test-time pose refinement of a held-out view against frozen scene networks (eval.py:824-858; SPARF's original loop is
// lib/bg_nerf/source/models/renderer.py:1312-1337 and :911-935): the two pieces of an iteration that are a dozen one-line
// elementwise launches in torch - the rays and targets of the drawn pixels, and the MSE with its gradient.  The network
// passes are pp_nerf_fwd / pp_nerf_bwd_input (pp_nerf.hip), the pose chain is pp_pose_fwd / pp_nerf_c2w_fold / pp_pose_bwd /
// pp_adam_flat; poseprobe_amd/pose_refine.py strings them together.
#include "pp_common.h"

// One thread per ray.  Pixel centre (idx % W + 0.5, idx / W + 0.5) (utils/camera.py:347-381); K = [fx s cx; 0 fy cy; 0 0 1]:
// K^-1 [x, y, 1] = ((x - cx - s * dy) / fx, dy = (y - cy) / fy, 1); ray = R dir_cam, center = t of c2w = [R | t]
// (utils/camera.py:384-416: cam2world(grid) - cam2world(0)).  An index outside [0, H * W) is clamped into it: the caller rules
// it out, and no read may leave the image.
__global__ __launch_bounds__(256) void k_nerf_rays_select(const float* __restrict__ c2w, const float* __restrict__ K,
                                                          const int32_t* __restrict__ ray_idx, int n, int H, int W,
                                                          const float* __restrict__ image, float* __restrict__ center,
                                                          float* __restrict__ ray, float* __restrict__ dir_cam,
                                                          float* __restrict__ target) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int idx = min(max(ray_idx[i], 0), H * W - 1);
  const int py = idx / W, px = idx - py * W;
  const float fx = K[0], s = K[1], cx = K[2], fy = K[4], cy = K[5];
  const float dy = ((float)py + 0.5f - cy) / fy;
  const float dx = ((float)px + 0.5f - cx - s * dy) / fx;
  const size_t o = (size_t)i * 3, p = (size_t)idx * 3;
  dir_cam[o] = dx; dir_cam[o + 1] = dy; dir_cam[o + 2] = 1.f;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    ray[o + r] = c2w[r * 4] * dx + c2w[r * 4 + 1] * dy + c2w[r * 4 + 2];
    center[o + r] = c2w[r * 4 + 3];
    target[o + r] = image[p + r];
  }
}

extern "C" int pp_nerf_rays_select(const float* c2w, const float* K, const int32_t* ray_idx, int32_t n_rays, int32_t H, int32_t W,
                                   const float* image, float* center, float* ray, float* dir_cam, float* target, void* stream) {
  PP_REQUIRE(c2w && K && ray_idx && image && center && ray && dir_cam && target, "null pointer");
  PP_REQUIRE(n_rays > 0 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 29), "bad sizes");
  hipLaunchKernelGGL(k_nerf_rays_select, dim3(pp_div_up(n_rays, 256)), dim3(256), 0, pp_stream(stream), c2w, K, ray_idx, n_rays, H, W,
                     image, center, ray, dir_cam, target);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// weight * mse_loss(pred, label, reduction = mean) and its gradient w.r.t. pred.  One work-group, fixed summation order
// (strided partial sums, then a tree over the 1024 partials), as k_nerf_huber.
__global__ __launch_bounds__(1024) void k_nerf_mse(const float* __restrict__ pred, const float* __restrict__ label, int n,
                                                   float weight, float* __restrict__ loss, float* __restrict__ g_pred) {
  __shared__ float red[1024];
  float acc = 0.f;
  const float gs = 2.f * weight / (float)n;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float d = pred[i] - label[i];
    acc += d * d;
    g_pred[i] = gs * d;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = weight * (red[0] / (float)n);
}

extern "C" int pp_nerf_mse_loss(const float* pred, const float* label, int32_t n, float weight, float* loss, float* g_pred,
                                void* stream) {
  PP_REQUIRE(pred && label && loss && g_pred, "null pointer");
  PP_REQUIRE(n > 0, "bad arguments");
  hipLaunchKernelGGL(k_nerf_mse, dim3(1), dim3(1024), 0, pp_stream(stream), pred, label, n, weight, loss, g_pred);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
