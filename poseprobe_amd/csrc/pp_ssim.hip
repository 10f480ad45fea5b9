// SSIM of image pairs (include/poseprobe_hip.h, pp_ssim_*; DESIGN.md "Image and pose scores"): lib/utils.py:792-838 (rgb_ssim) on
// device-resident channels-last images.
//
//   filter     the 1-D Gaussian of :804-808, computed on the host in fp64 and handed to the kernel by value, unrounded: rounded to
//              fp32 the 11-tap filter sums to 1 - 1.4e-9, which gives a constant image the variance 2.8e-9 against c2 = 9e-4 -
//              3e-6 of the score of a black against a white image, 26 fp32 ulps.
//   tiles      one work-group (256 threads, four wavefronts) takes one SSIM_T x SSIM_T output tile of one view with all its
//              channels.  It stages the (SSIM_T + fs - 1)^2 window of both images in LDS once - a window row is one contiguous
//              run of C (SSIM_T + fs - 1) floats of the image -, then per channel runs the row pass of the five moment images
//              (x, y, xx, yy, xy) into LDS and the column pass with its accumulators in registers.  When the window of all channels
//              does not fit the LDS budget (large filters) it is staged one channel at a time instead.
//   arithmetic fp32 inputs; products, sums (one fused multiply-add per tap) and the per-pixel formula in fp64, rounded once to
//              fp32 for the map.  The variances cancel (E[xx] - E[x]^2): fp32 sums would leave an error of 1e-7 against c2 = 9e-4.
//   mean       no atomics: a group adds its tile in a fixed order and writes the fp64 sum to its own slot; k_ssim_finish adds a
//              view's slots in a fixed order.  A view's value does not depend on the batch it is in.
#include <math.h>

#include "pp_common.h"

namespace {

constexpr int SSIM_T = 16;                       // output tile edge
constexpr int SSIM_THREADS = SSIM_T * SSIM_T;    // one thread per output pixel of the tile in the column pass
constexpr int SSIM_FS_MAX = 33;
constexpr int SSIM_LDS_BUDGET = 64 * 1024 - 64;  // bytes of dynamic LDS per work-group (the fold of the four wavefronts' sums takes 32 more)

struct SsimArgs {
  double w[SSIM_FS_MAX];
  int fs;
  double c1, c2;
};

// bytes of LDS of one group: row-pass results fp64 [5][WR][T] + both windows fp32 [2][WR][WR cw]
size_t ssim_lds_bytes(int fs, int cw) {
  const size_t WR = SSIM_T + fs - 1;
  return 8 * 5 * WR * SSIM_T + 4 * 2 * WR * WR * cw;
}

__global__ __launch_bounds__(SSIM_THREADS) void k_ssim_tiles(const float* __restrict__ img0, const float* __restrict__ img1, int H, int W,
                                                             int C, int tiles_x, int tiles_per_view, int cw, SsimArgs a,
                                                             double* __restrict__ partial, float* __restrict__ map) {
  extern __shared__ double ssim_lds[];
  __shared__ double red[SSIM_THREADS / 64];
  const int fs = a.fs, WR = SSIM_T + fs - 1, plane = WR * SSIM_T, run = WR * cw;
  double* rowbuf = ssim_lds;                                   // [5][WR][T]
  float* win0 = reinterpret_cast<float*>(rowbuf + 5 * plane);  // [WR][WR][cw]
  float* win1 = win0 + WR * run;
  const int tid = threadIdx.x;
  const int v = blockIdx.x / tiles_per_view, t = blockIdx.x % tiles_per_view;
  const int r0 = (t / tiles_x) * SSIM_T, c0 = (t % tiles_x) * SSIM_T;
  const int OH = H - fs + 1, OW = W - fs + 1;
  const size_t base = (size_t)v * H * W * C;
  const int oi = tid / SSIM_T, oj = tid % SSIM_T;
  const bool live = r0 + oi < OH && c0 + oj < OW;
  double acc = 0.0;
  for (int cb = 0; cb < C; cb += cw) {
    __syncthreads();                                           // the previous chunk's readers are done
    for (int idx = tid; idx < WR * run; idx += SSIM_THREADS) {
      const int r = idx / run, e = idx % run;
      const int gr = r0 + r, gc = c0 + e / cw;
      float x = 0.0f, y = 0.0f;                                // (outside the image: feeds only outputs that are not kept)
      if (gr < H && gc < W) {
        const size_t o = base + ((size_t)gr * W + gc) * C + cb + e % cw;
        x = img0[o];
        y = img1[o];
      }
      win0[idx] = x;
      win1[idx] = y;
    }
    __syncthreads();
    for (int c = 0; c < cw; ++c) {
      if (c > 0) __syncthreads();                              // the previous channel's column pass is done with rowbuf
      for (int idx = tid; idx < plane; idx += SSIM_THREADS) {
        const int r = idx / SSIM_T, j = idx % SSIM_T;
        const float* p0 = win0 + r * run + j * cw + c;
        const float* p1 = win1 + r * run + j * cw + c;
        double s0 = 0.0, s1 = 0.0, s00 = 0.0, s11 = 0.0, s01 = 0.0;
        for (int k = 0; k < fs; ++k) {
          const double w = a.w[k], x = p0[k * cw], y = p1[k * cw];
          s0 = fma(w, x, s0);
          s1 = fma(w, y, s1);
          s00 = fma(w, x * x, s00);                            // (x x, y y, x y: products of fp32 values, exact in fp64)
          s11 = fma(w, y * y, s11);
          s01 = fma(w, x * y, s01);
        }
        rowbuf[idx] = s0;
        rowbuf[plane + idx] = s1;
        rowbuf[2 * plane + idx] = s00;
        rowbuf[3 * plane + idx] = s11;
        rowbuf[4 * plane + idx] = s01;
      }
      __syncthreads();
      double m0 = 0.0, m1 = 0.0, e00 = 0.0, e11 = 0.0, e01 = 0.0;
      const double* q = rowbuf + oi * SSIM_T + oj;
      for (int k = 0; k < fs; ++k) {
        const double w = a.w[k];
        const double* qk = q + k * SSIM_T;
        m0 = fma(w, qk[0], m0);
        m1 = fma(w, qk[plane], m1);
        e00 = fma(w, qk[2 * plane], e00);
        e11 = fma(w, qk[3 * plane], e11);
        e01 = fma(w, qk[4 * plane], e01);
      }
      const double mu00 = m0 * m0, mu11 = m1 * m1, mu01 = m0 * m1;
      const double v00 = fmax(0.0, e00 - mu00), v11 = fmax(0.0, e11 - mu11);
      double v01 = e01 - mu01;
      const double lim = fmin(sqrt(v00 * v11), fabs(v01));
      v01 = v01 > 0.0 ? lim : v01 < 0.0 ? -lim : v01 * lim;    // sign(v01) min(.., |v01|)
      const double val = ((2.0 * mu01 + a.c1) * (2.0 * v01 + a.c2)) / ((mu00 + mu11 + a.c1) * (v00 + v11 + a.c2));
      if (live) {
        acc += val;
        if (map) map[(((size_t)v * OH + (r0 + oi)) * OW + (c0 + oj)) * C + cb + c] = (float)val;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
#pragma unroll
    for (int k = 1; k < SSIM_THREADS / 64; ++k) s += red[k];
    partial[blockIdx.x] = s;
  }
}

// one wavefront per view: lane l adds slots l, l + 64, ... in ascending order, then the lanes are folded
__global__ __launch_bounds__(64) void k_ssim_finish(const double* __restrict__ partial, int tiles_per_view, double count,
                                                    float* __restrict__ out) {
  const int v = blockIdx.x, lane = threadIdx.x;
  const double* p = partial + (size_t)v * tiles_per_view;
  double s = 0.0;
  for (int i = lane; i < tiles_per_view; i += 64) s += p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) out[v] = (float)(s / count);
}

// shared argument checks; tiles = output tiles of one view
int ssim_shape(const char* fn, int32_t V, int32_t H, int32_t W, int32_t filter_size, int64_t& tiles_x, int64_t& tiles) {
  if (V < 1) { pp_set_error("%s: at least one view", fn); return PP_ERR_INVALID_ARG; }
  if (filter_size < 1 || filter_size > SSIM_FS_MAX) {
    pp_set_error("%s: filter_size %d outside 1..%d", fn, filter_size, SSIM_FS_MAX);
    return PP_ERR_INVALID_ARG;
  }
  if (H < filter_size || W < filter_size) {
    pp_set_error("%s: a %d x %d image is smaller than the filter (%d)", fn, H, W, filter_size);
    return PP_ERR_INVALID_ARG;
  }
  tiles_x = ((int64_t)W - filter_size + SSIM_T) / SSIM_T;
  tiles = tiles_x * (((int64_t)H - filter_size + SSIM_T) / SSIM_T);
  if (tiles * V >= (1ll << 31)) {
    pp_set_error("%s: %lld output tiles: at most 2^31 - 1 (one work-group each)", fn, (long long)(tiles * V));
    return PP_ERR_UNSUPPORTED;
  }
  return PP_OK;
}

}  // namespace

extern "C" int pp_ssim_tile(int32_t* tile) {
  PP_REQUIRE(tile, "null pointer");
  *tile = SSIM_T;
  return PP_OK;
}

extern "C" int pp_ssim_workspace(int32_t V, int32_t H, int32_t W, int32_t filter_size, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  int64_t tiles_x, tiles;
  if (int rc = ssim_shape(__func__, V, H, W, filter_size, tiles_x, tiles)) return rc;
  *bytes = 8 * tiles * V;
  return PP_OK;
}

extern "C" int pp_ssim(const float* img0, const float* img1, int32_t V, int32_t H, int32_t W, int32_t C, int32_t filter_size,
                       double filter_sigma, double max_val, double k1, double k2, void* work, int64_t work_bytes, float* ssim,
                       float* map, void* stream) {
  PP_REQUIRE(img0 && img1 && work && ssim, "null pointer");
  PP_REQUIRE(C >= 1 && C <= 4, "1 to 4 channels");
  int64_t tiles_x, tiles;
  if (int rc = ssim_shape(__func__, V, H, W, filter_size, tiles_x, tiles)) return rc;
  PP_REQUIRE(filter_sigma > 0.0 && filter_sigma - filter_sigma == 0.0, "filter_sigma must be positive and finite");
  PP_REQUIRE(max_val > 0.0 && max_val - max_val == 0.0, "max_val must be positive and finite");
  PP_REQUIRE(k1 - k1 == 0.0 && k2 - k2 == 0.0, "k1 and k2 must be finite");
  PP_REQUIRE(work_bytes >= 8 * tiles * V, "workspace too small (pp_ssim_workspace)");
  PP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7) == 0, "workspace must be 8-byte aligned");
  SsimArgs a;
  memset(&a, 0, sizeof(a));
  a.fs = filter_size;
  {                                                            // lib/utils.py:804-808
    const int hw = filter_size / 2;
    const double shift = (2 * hw - filter_size + 1) / 2.0;
    double f[SSIM_FS_MAX], sum = 0.0;
    for (int k = 0; k < filter_size; ++k) {
      const double u = (k - hw + shift) / filter_sigma;
      f[k] = exp(-0.5 * (u * u));
      sum += f[k];
    }
    for (int k = 0; k < filter_size; ++k) a.w[k] = f[k] / sum;
  }
  a.c1 = (k1 * max_val) * (k1 * max_val);
  a.c2 = (k2 * max_val) * (k2 * max_val);
  const int cw = ssim_lds_bytes(filter_size, C) <= (size_t)SSIM_LDS_BUDGET ? C : 1;
  hipStream_t st = pp_stream(stream);
  double* partial = static_cast<double*>(work);
  hipLaunchKernelGGL(k_ssim_tiles, dim3((unsigned)(tiles * V)), dim3(SSIM_THREADS), ssim_lds_bytes(filter_size, cw), st, img0, img1, H, W,
                     C, (int)tiles_x, (int)tiles, cw, a, partial, map);
  hipLaunchKernelGGL(k_ssim_finish, dim3(V), dim3(64), 0, st, partial, (int)tiles,
                     (double)(H - filter_size + 1) * (double)(W - filter_size + 1) * (double)C, ssim);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
