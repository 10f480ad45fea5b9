// Layer-by-layer kernels of the object-branch MLPs, exact fp32 (v_mfma_f32_32x32x2_f32): a persistent NT GEMM (pp_gemm.h:
// work-group = 4 wavefronts in 2x2, 64-row x 128-feature tile, K-chunks of 32 through LDS rows of 36 floats so that a lane fetches
// its four operands of consecutive MFMAs with one ds_read_b128; next chunk / next tile prefetched into registers behind the MFMA
// block), a split-K TN GEMM for the weight gradients and the thin first / last layers.  They serve generic MLP shapes (DirectVoxGO
// twin) and A/B runs (option mlp_fused = 0); the Voxurf shapes run through the layer-fused kernels of pp_mlp_fused.hip and
// pp_mlp_split.hip.  In the accumulator layout a lane holds ONE feature column and rows (reg&3) + 8*(reg>>2) + 4*(lane>>5): the
// four rows of a warp sample (pp_mlp.hip) are registers 4q..4q+3 of the same lane, so the 4-row masking needs no cross-lane traffic.
#include "pp_common.h"
#include "pp_mlp_fused.h"

#include "pp_gemm.h"

// dst[c][r] = src[r][c]  (weights are tiny: 128x128 / 128x64); lets the backward-data GEMM run in the same NT form
static __global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  int c = i / rows, r = i - c * rows;           // consecutive threads write consecutive dst elements
  dst[i] = src[r * cols + c];
}

// ------------------------------------------------------------------------------------------------ small layers
// warp layer 0 (3 -> 128) in 4-row form.  block = 2 samples x 128 features.
__global__ __launch_bounds__(256) void k_warp_l0_fwd(const float* __restrict__ W0, const float* __restrict__ b0,
                                                     const float* __restrict__ pts, const int32_t* __restrict__ count,
                                                     int capacity, float* __restrict__ X1) {
  int M = min(count[0], capacity);
  int m = blockIdx.x * 2 + (threadIdx.x >> 7), j = threadIdx.x & 127;
  if (m >= M) return;
  float w0 = W0[j * 3], w1 = W0[j * 3 + 1], w2 = W0[j * 3 + 2];
  float y = pts[m * 3] * w0 + pts[m * 3 + 1] * w1 + pts[m * 3 + 2] * w2 + b0[j];
  bool on = y > 0.f;
  size_t base = (size_t)m * 4 * 128 + j;
  X1[base] = on ? y : 0.f;
  X1[base + 128] = on ? w0 : 0.f;
  X1[base + 256] = on ? w1 : 0.f;
  X1[base + 384] = on ? w2 : 0.f;
}

// warp output layer (128 -> 4) on 4 rows: one wavefront per sample, 16 lanes per row.
__global__ __launch_bounds__(256) void k_warp_l4_fwd(const float* __restrict__ W4, const float* __restrict__ b4,
                                                     const float* __restrict__ X4, const int32_t* __restrict__ count,
                                                     int capacity, float out_range, float* __restrict__ out) {
  int M = min(count[0], capacity);
  int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  int c = lane >> 4, sub = lane & 15;
  const float4* xp = reinterpret_cast<const float4*>(X4 + ((size_t)m * 4 + c) * 128 + sub * 8);
  float4 xa = xp[0], xb = xp[1];
  float acc[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float4* wp = reinterpret_cast<const float4*>(W4 + o * 128 + sub * 8);
    float4 wa = wp[0], wb = wp[1];
    float s = xa.x * wa.x + xa.y * wa.y + xa.z * wa.z + xa.w * wa.w + xb.x * wb.x + xb.y * wb.y + xb.z * wb.z + xb.w * wb.w;
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    acc[o] = s;
  }
  if (sub == 0) {
    float4 r;
    r.x = (acc[0] + (c == 0 ? b4[0] : 0.f)) * out_range;
    r.y = (acc[1] + (c == 0 ? b4[1] : 0.f)) * out_range;
    r.z = (acc[2] + (c == 0 ? b4[2] : 0.f)) * out_range;
    r.w = (acc[3] + (c == 0 ? b4[3] : 0.f)) * out_range;
    *reinterpret_cast<float4*>(out + (size_t)m * 16 + c * 4) = r;
  }
}

// backward of the output layer: Ybar4 = mask(X4) * (out_grad*range) W4 ; W4bar, b4bar accumulated over a strip.
#define STRIP 64
__global__ __launch_bounds__(256) void k_warp_l4_bwd(const float* __restrict__ W4, const float* __restrict__ X4,
                                                     const float* __restrict__ out_grad,
                                                     const int32_t* __restrict__ count, int capacity, float out_range,
                                                     float* __restrict__ Ybar, float* __restrict__ W4bar,
                                                     float* __restrict__ b4bar) {
  __shared__ float red[4 * 128];
  int M = min(count[0], capacity);
  int m0 = blockIdx.x * STRIP;
  if (m0 >= M) return;
  int h = threadIdx.x >> 7, j = threadIdx.x & 127;
  float w[4] = {W4[j], W4[128 + j], W4[256 + j], W4[384 + j]};
  float wacc[4] = {0, 0, 0, 0}, bacc = 0.f;
  int mend = min(m0 + STRIP, M);
  for (int m = m0 + h; m < mend; m += 2) {
    const float* og = out_grad + (size_t)m * 16;
    size_t base = (size_t)m * 4 * 128 + j;
    bool on = X4[base] > 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float g0 = og[c * 4] * out_range, g1 = og[c * 4 + 1] * out_range, g2 = og[c * 4 + 2] * out_range,
            g3 = og[c * 4 + 3] * out_range;
      float x = X4[base + c * 128];
      wacc[0] += g0 * x; wacc[1] += g1 * x; wacc[2] += g2 * x; wacc[3] += g3 * x;
      float xb = g0 * w[0] + g1 * w[1] + g2 * w[2] + g3 * w[3];
      Ybar[base + c * 128] = on ? xb : 0.f;
    }
    if (j < 4) bacc += og[j] * out_range;
  }
  if (h == 1) { for (int o = 0; o < 4; ++o) red[o * 128 + j] = wacc[o]; }
  __syncthreads();
  if (h == 0) { for (int o = 0; o < 4; ++o) atomicAdd(&W4bar[o * 128 + j], wacc[o] + red[o * 128 + j]); }
  if (j < 4 && bacc != 0.f) atomicAdd(&b4bar[j], bacc);
}

// backward of warp layer 0, part (a): pts_grad[m][i] += sum_j Ybar1[4m][j] * W0[j][i]   (16 lanes per sample)
__global__ __launch_bounds__(256) void k_warp_l0_bwd_pts(const float* __restrict__ W0, const float* __restrict__ Ybar,
                                                         const int32_t* __restrict__ count, int capacity,
                                                         float* __restrict__ pts_grad) {
  int M = min(count[0], capacity);
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int m = t >> 4, sub = t & 15;
  bool live = m < M;
  float acc[3] = {0.f, 0.f, 0.f};
  if (live) {
    const float4* yp = reinterpret_cast<const float4*>(Ybar + (size_t)m * 4 * 128 + sub * 8);
    float4 ya = yp[0], yb = yp[1];
    float y[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float* w = W0 + (sub * 8 + q) * 3;
      acc[0] += y[q] * w[0]; acc[1] += y[q] * w[1]; acc[2] += y[q] * w[2];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float v = acc[i];
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 1, 64);
    if (live && sub == 0) pts_grad[m * 3 + i] += v;
  }
}

// part (b): W0bar[j][i] += sum_m (Ybar1[4m][j] p_i + Ybar1[4m+1+i][j]) ; b0bar[j] += sum_m Ybar1[4m][j]
#define STRIP0 128
__global__ __launch_bounds__(256) void k_warp_l0_bwd_w(const float* __restrict__ pts, const float* __restrict__ Ybar,
                                                       const int32_t* __restrict__ count, int capacity,
                                                       float* __restrict__ W0bar, float* __restrict__ b0bar) {
  __shared__ float red[4 * 128];
  int M = min(count[0], capacity);
  int m0 = blockIdx.x * STRIP0;
  if (m0 >= M) return;
  int h = threadIdx.x >> 7, j = threadIdx.x & 127;
  float wacc[3] = {0, 0, 0}, bacc = 0.f;
  int mend = min(m0 + STRIP0, M);
  for (int m = m0 + h; m < mend; m += 2) {
    size_t base = (size_t)m * 4 * 128 + j;
    float y0 = Ybar[base];
    wacc[0] += y0 * pts[m * 3] + Ybar[base + 128];
    wacc[1] += y0 * pts[m * 3 + 1] + Ybar[base + 256];
    wacc[2] += y0 * pts[m * 3 + 2] + Ybar[base + 384];
    bacc += y0;
  }
  if (h == 1) { for (int i = 0; i < 3; ++i) red[i * 128 + j] = wacc[i]; red[3 * 128 + j] = bacc; }
  __syncthreads();
  if (h == 0) {
    for (int i = 0; i < 3; ++i) atomicAdd(&W0bar[j * 3 + i], wacc[i] + red[i * 128 + j]);
    atomicAdd(&b0bar[j], bacc + red[3 * 128 + j]);
  }
}

// rgbnet output layer (128 -> 3) + sigmoid: 16 lanes per sample.
__global__ __launch_bounds__(256) void k_rgb_out_fwd(const float* __restrict__ W3, const float* __restrict__ b3,
                                                     const float* __restrict__ H3, const int32_t* __restrict__ count,
                                                     int capacity, const float* __restrict__ logit_add, int add_ld,
                                                     float* __restrict__ rgb) {
  int M = min(count[0], capacity);
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  int m = t >> 4, sub = t & 15;
  bool live = m < M;
  float4 xa = make_float4(0, 0, 0, 0), xb = xa;
  if (live) {
    const float4* xp = reinterpret_cast<const float4*>(H3 + (size_t)m * 128 + sub * 8);
    xa = xp[0]; xb = xp[1];
  }
  float acc[3];
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    const float4* wp = reinterpret_cast<const float4*>(W3 + o * 128 + sub * 8);
    float4 wa = wp[0], wb = wp[1];
    float s = xa.x * wa.x + xa.y * wa.y + xa.z * wa.z + xa.w * wa.w + xb.x * wb.x + xb.y * wb.y + xb.z * wb.z + xb.w * wb.w;
    s += __shfl_xor(s, 8, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 1, 64);
    acc[o] = s;
  }
  if (live && sub == 0)
    for (int o = 0; o < 3; ++o) rgb[m * 3 + o] = pp_sigmoid(acc[o] + b3[o] + (logit_add ? logit_add[(size_t)m * add_ld + o] : 0.f));
}

__global__ __launch_bounds__(256) void k_rgb_out_bwd(const float* __restrict__ W3, const float* __restrict__ H3,
                                                     const float* __restrict__ rgb, const float* __restrict__ rgb_grad,
                                                     const int32_t* __restrict__ count, int capacity,
                                                     float* __restrict__ Ybar, float* __restrict__ W3bar,
                                                     float* __restrict__ b3bar, float* __restrict__ logit_grad, int lg_ld) {
  __shared__ float red[3 * 128];
  int M = min(count[0], capacity);
  int m0 = blockIdx.x * STRIP;
  if (m0 >= M) return;
  int h = threadIdx.x >> 7, j = threadIdx.x & 127;
  float w[3] = {W3[j], W3[128 + j], W3[256 + j]};
  float wacc[3] = {0, 0, 0}, bacc = 0.f;
  int mend = min(m0 + STRIP, M);
  for (int m = m0 + h; m < mend; m += 2) {
    float gl[3];
#pragma unroll
    for (int o = 0; o < 3; ++o) { float r = rgb[m * 3 + o]; gl[o] = rgb_grad[m * 3 + o] * r * (1.f - r); }
    float x = H3[(size_t)m * 128 + j];
    wacc[0] += gl[0] * x; wacc[1] += gl[1] * x; wacc[2] += gl[2] * x;
    float hb = gl[0] * w[0] + gl[1] * w[1] + gl[2] * w[2];
    Ybar[(size_t)m * 128 + j] = (x > 0.f) ? hb : 0.f;
    if (j < 3) { bacc += gl[j]; if (logit_grad) logit_grad[(size_t)m * lg_ld + j] = gl[j]; }
  }
  if (h == 1) { for (int o = 0; o < 3; ++o) red[o * 128 + j] = wacc[o]; }
  __syncthreads();
  if (h == 0) { for (int o = 0; o < 3; ++o) atomicAdd(&W3bar[o * 128 + j], wacc[o] + red[o * 128 + j]); }
  if (j < 3 && bacc != 0.f) atomicAdd(&b3bar[j], bacc);
}

// ------------------------------------------------------------------------------------------------ host side
// (parameter-block offsets of the two nets: WPF_* / RGF_* of pp_mlp_fused.h)
// weight-gradient GEMM: a FIXED number of work-groups splits the (device-side) row count evenly; measured optimum on
// MI355X ~ 450 work-groups (more: the 64 KB of contended atomics per work-group dominates; fewer: idle CUs).
static const int TN_WGS = 448;

static const int GEMM_MAX_WG = 256 * 5;     // 5 resident work-groups per CU at BM=64 (25 KB LDS, 90 regs)
static inline int gemm_grid(int rows, int bm) {
  int t = pp_div_up(rows, bm);
  return t < GEMM_MAX_WG ? t : GEMM_MAX_WG;
}
#define PP_GEMM_BM 64

// Generic ReLU MLP  in_ld -> 128 -> ... -> 128 -> 3 (+ optional sigmoid), n_gemm = number of 128-wide hidden layers.
// Parameter block: W0[128*in_ld] b0[128] | (W[128*128] b[128]) x (n_gemm-1) | Wout[3*128] bout[3].
static inline size_t mlp_off_hidden(int in_ld, int l) { return (size_t)128 * in_ld + 128 + (size_t)(l - 1) * (128 * 128 + 128); }
static inline size_t mlp_off_out(int in_ld, int n_gemm) { return mlp_off_hidden(in_ld, n_gemm); }

void pp_launch_mlp_layered_fwd(const float* params, const float* feat, int in_ld, int n_gemm, const int32_t* count, int capacity,
                               const float* logit_add, int logit_add_ld, float* acts, float* out, hipStream_t st) {
  const size_t LS = (size_t)capacity * 128;
  dim3 g(gemm_grid(capacity, PP_GEMM_BM)), b(256);
  hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_RELU, 1, PP_GEMM_BM>), g, b, 0, st, feat, in_ld, params, in_ld, in_ld, 128,
                     params + (size_t)128 * in_ld, nullptr, 0, acts, 128, count, 1, capacity);
  for (int l = 1; l < n_gemm; ++l) {
    const float* W = params + mlp_off_hidden(in_ld, l);
    hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_RELU, 1, PP_GEMM_BM>), g, b, 0, st, acts + (l - 1) * LS, 128, W, 128, 128, 128,
                       W + 128 * 128, nullptr, 0, acts + l * LS, 128, count, 1, capacity);
  }
  const float* Wo = params + mlp_off_out(in_ld, n_gemm);
  hipLaunchKernelGGL(k_rgb_out_fwd, dim3(pp_div_up(capacity * 16, 256)), b, 0, st, Wo, Wo + 3 * 128,
                     acts + (n_gemm - 1) * LS, count, capacity, logit_add, logit_add_ld, out);
}

void pp_launch_mlp_layered_bwd(const float* params, const float* feat, int in_ld, int n_gemm, const float* acts, const float* out,
                               const float* out_grad, const int32_t* count, int capacity, float* scratch, float* params_grad,
                               float* feat_grad, float* logit_add_grad, int logit_add_ld, hipStream_t st) {
  const size_t LS = (size_t)capacity * 128;
  float* cur = scratch;
  float* nxt = scratch + LS;
  float* wt = scratch + 2 * LS;      // one transposed weight matrix at a time (128*128 floats)
  dim3 g(gemm_grid(capacity, PP_GEMM_BM)), gt(TN_WGS), b(256);
  const size_t oo = mlp_off_out(in_ld, n_gemm);
  hipLaunchKernelGGL(k_rgb_out_bwd, dim3(pp_div_up(capacity, STRIP)), b, 0, st, params + oo, acts + (n_gemm - 1) * LS, out,
                     out_grad, count, capacity, cur, params_grad + oo, params_grad + oo + 3 * 128, logit_add_grad,
                     logit_add_ld);
  for (int l = n_gemm - 1; l >= 1; --l) {
    const size_t ow = mlp_off_hidden(in_ld, l);
    hipLaunchKernelGGL((k_gemm_tn<1>), gt, b, 0, st, cur, 128, acts + (l - 1) * LS, 128, 128, params_grad + ow, 128,
                       params_grad + ow + 128 * 128, count, 1, capacity);
    hipLaunchKernelGGL(k_transpose, dim3(64), b, 0, st, params + ow, wt, 128, 128);
    hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_MASK, 1, PP_GEMM_BM>), g, b, 0, st, cur, 128, wt, 128, 128, 128, nullptr,
                       acts + (l - 1) * LS, 128, nxt, 128, count, 1, capacity);
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  hipLaunchKernelGGL((k_gemm_tn<1>), gt, b, 0, st, cur, 128, feat, in_ld, in_ld, params_grad, in_ld,
                     params_grad + (size_t)128 * in_ld, count, 1, capacity);
  if (feat_grad) {
    hipLaunchKernelGGL(k_transpose, dim3(pp_div_up(128 * in_ld, 256)), b, 0, st, params, wt, 128, in_ld);
    hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_PLAIN, 1, PP_GEMM_BM>), g, b, 0, st, cur, 128, wt, 128, 128, in_ld, nullptr,
                       nullptr, 0, feat_grad, in_ld, count, 1, capacity);
  }
}

void pp_launch_warp_layered_fwd(const float* params, const float* pts, const int32_t* count, int capacity, float out_range,
                                float* acts, float* out, hipStream_t st) {
  const int rcap = capacity * 4;
  const size_t LS = (size_t)rcap * 128;
  dim3 g(gemm_grid(rcap, PP_GEMM_BM)), b(256);
  hipLaunchKernelGGL(k_warp_l0_fwd, dim3(pp_div_up(capacity, 2)), b, 0, st, params + WPF_W0, params + WPF_B0, pts, count,
                     capacity, acts);
  hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_RELU, 4, PP_GEMM_BM>), g, b, 0, st, acts, 128, params + WPF_W1, 128, 128, 128,
                     params + WPF_B1, nullptr, 0, acts + LS, 128, count, 4, rcap);
  hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_RELU, 4, PP_GEMM_BM>), g, b, 0, st, acts + LS, 128, params + WPF_W2, 128, 128, 128,
                     params + WPF_B2, nullptr, 0, acts + 2 * LS, 128, count, 4, rcap);
  hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_RELU, 4, PP_GEMM_BM>), g, b, 0, st, acts + 2 * LS, 128, params + WPF_W3, 128, 128, 128,
                     params + WPF_B3, nullptr, 0, acts + 3 * LS, 128, count, 4, rcap);
  hipLaunchKernelGGL(k_warp_l4_fwd, dim3(pp_div_up(capacity, 4)), b, 0, st, params + WPF_W4, params + WPF_B4,
                     acts + 3 * LS, count, capacity, out_range, out);
}

void pp_launch_warp_layered_bwd(const float* params, const float* pts, const float* acts, const float* out_grad, const int32_t* count,
                                int capacity, float out_range, float* scratch, float* params_grad, float* pts_grad, hipStream_t st) {
  const int rcap = capacity * 4;
  const size_t LS = (size_t)rcap * 128;
  float* cur = scratch;
  float* nxt = scratch + LS;
  float* wt = scratch + 2 * LS;          // transposed weights W3^T, W2^T, W1^T
  dim3 g(gemm_grid(rcap, PP_GEMM_BM)), gt(TN_WGS), b(256);
  hipLaunchKernelGGL(k_transpose, dim3(64), b, 0, st, params + WPF_W3, wt, 128, 128);
  hipLaunchKernelGGL(k_transpose, dim3(64), b, 0, st, params + WPF_W2, wt + 16384, 128, 128);
  hipLaunchKernelGGL(k_transpose, dim3(64), b, 0, st, params + WPF_W1, wt + 32768, 128, 128);
  hipLaunchKernelGGL(k_warp_l4_bwd, dim3(pp_div_up(capacity, STRIP)), b, 0, st, params + WPF_W4, acts + 3 * LS, out_grad,
                     count, capacity, out_range, cur, params_grad + WPF_W4, params_grad + WPF_B4);
  const int w_off[4] = {0, WPF_W1, WPF_W2, WPF_W3};
  const int b_off[4] = {0, WPF_B1, WPF_B2, WPF_B3};
  for (int l = 3; l >= 1; --l) {
    hipLaunchKernelGGL((k_gemm_tn<4>), gt, b, 0, st, cur, 128, acts + (l - 1) * LS, 128, 128, params_grad + w_off[l], 128,
                       params_grad + b_off[l], count, 4, rcap);
    hipLaunchKernelGGL((k_gemm128<MODE_NT, EPI_MASK, 4, PP_GEMM_BM>), g, b, 0, st, cur, 128, wt + (3 - l) * 16384, 128, 128,
                       128, nullptr, acts + (l - 1) * LS, 128, nxt, 128, count, 4, rcap);
    float* tmp = cur; cur = nxt; nxt = tmp;
  }
  // layer 0 (cur = Ybar1)
  hipLaunchKernelGGL(k_warp_l0_bwd_pts, dim3(pp_div_up(capacity * 16, 256)), b, 0, st, params + WPF_W0, cur, count, capacity,
                     pts_grad);
  hipLaunchKernelGGL(k_warp_l0_bwd_w, dim3(pp_div_up(capacity, STRIP0)), b, 0, st, pts, cur, count, capacity,
                     params_grad + WPF_W0, params_grad + WPF_B0);
}
