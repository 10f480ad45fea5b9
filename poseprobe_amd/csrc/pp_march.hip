// Transmittance scan (alpha -> weights) and fused compositing, forward and backward.
// One wavefront per ray: lanes hold 64 consecutive samples (coalesced), the running transmittance is advanced in
// the reference's *sequential* order inside the wave (v_readlane broadcast), so the 1e-3 early stop and every
// rounding of lib/cuda/render_utils_kernel.cu:577-605 / :654-707 are reproduced exactly while memory traffic is
// coalesced (the reference walks each ray from a single thread).
#include "pp_common.h"
#include "pp_loss_body.h"

// value of lane j (j wave-uniform): v_readlane_b32 instead of the ds_bpermute_b32 that __shfl compiles to - inside the sequential
// loops below an LDS crossbar round trip per sample was most of the iteration (k_march_fwd 17.6 us for a 186-sample ray)
__device__ __forceinline__ float lane_value(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ __forceinline__ double lane_value(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// ---- the per-chunk / per-ray steps of both directions, shared by the stand-alone kernels and k_march_loss_bwd ----------------
struct MarchAcc {
  float Tc = 1.f;
  int stop;                // absolute index one past the last sample that received a weight
  bool stopped = false;
  float rgb[3] = {0, 0, 0}, w = 0.f, d = 0.f, n[3] = {0, 0, 0};
};

// one chunk of 64 samples starting at c0: lane's sample is c0 + lane, `a` its alpha (0 past the end), cr / cs / cn its colour, step
// weight and normal (0 where absent).  Leaves the lane's transmittance and weight in myT / myw and adds to the ray's sums.
template <bool FUSED, bool DVGO>
__device__ __forceinline__ void march_fwd_chunk(MarchAcc& s, const int c0, const int e, const int lane, const float a,
                                                const bool has_rgb, const float (&cr)[3], const bool has_sw, const float cs,
                                                const bool has_n, const float (&cn)[3], float& myT, float& myw) {
  myT = 1.f; myw = 0.f;
  if (!s.stopped) {
    int n = e - c0 < 64 ? e - c0 : 64;
    // the transmittance is a sequential product; a sample's factor (1 - alpha, in double for the reference's arithmetic) is
    // formed by its own lane before the loop, and its weight T * alpha after it: the serial part is one multiply per sample
    const double omd = 1.0 - (double)a;
    const float omf = fmaxf(1.f - a, 1e-10f);
    bool reached = false;
    for (int j = 0; j < n; ++j) {
      if (lane == j) { myT = s.Tc; reached = true; }
      if (DVGO) {           // cumprod_exclusive: p.clamp_min(1e-10).cumprod(-1), fp32, no early stop (dvgo_ori.py:478-485)
        s.Tc = s.Tc * lane_value(omf, j);
      } else {
        s.Tc = (float)((double)s.Tc * lane_value(omd, j));
        if (s.Tc < 1e-3f) { s.stop = c0 + j + 1; s.stopped = true; break; }   // == ((double)Tc < 1e-3): float(1e-3) is the first float above it
      }
    }
    if (reached) myw = myT * a;
  }
  if (FUSED && c0 + lane < e) {
    s.w += myw;
    if (has_rgb) for (int k = 0; k < 3; ++k) s.rgb[k] += myw * cr[k];
    if (has_sw) s.d += myw * cs;
    if (has_n) for (int k = 0; k < 3; ++k) s.n[k] += myw * cn[k];
  }
}

// the ray's sums over the wavefront and its outputs (lane 0 stores); pre / rgbm: the composited colour before / after the clamp
template <bool FUSED>
__device__ __forceinline__ void march_fwd_finish(MarchAcc& s, const int r, const int lane, const float bg,
                                                 float* __restrict__ alphainv_last, int32_t* __restrict__ i_end,
                                                 float* __restrict__ rgb_marched, float* __restrict__ rgb_pre,
                                                 float* __restrict__ cum_weights, float* __restrict__ depth_acc,
                                                 float* __restrict__ normal_marched, float (&pre)[3], float (&rgbm)[3]) {
  if (FUSED) {
    s.w = pp_wave_sum(s.w);
    s.d = pp_wave_sum(s.d);
    for (int k = 0; k < 3; ++k) { s.rgb[k] = pp_wave_sum(s.rgb[k]); s.n[k] = pp_wave_sum(s.n[k]); }
    for (int k = 0; k < 3; ++k) {
      pre[k] = s.rgb[k] + (1.f - s.w) * bg;
      rgbm[k] = fminf(fmaxf(pre[k], 0.f), 1.f);
    }
  }
  if (lane == 0) {
    alphainv_last[r] = s.Tc;
    i_end[r] = s.stop;
    if (FUSED) {
      cum_weights[r] = s.w;
      if (depth_acc) depth_acc[r] = s.d;
      for (int k = 0; k < 3; ++k) {
        if (rgb_pre) rgb_pre[r * 3 + k] = pre[k];
        if (rgb_marched) rgb_marched[r * 3 + k] = rgbm[k];
        if (normal_marched) normal_marched[r * 3 + k] = s.n[k];
      }
    }
  }
}

// backward, per ray: the clamp mask on the colour gradient and the gradient of the weight sum
__device__ __forceinline__ void march_bwd_ray(const float (&pre)[3], const float (&g)[3], const float g_cw, const float bg,
                                              float (&gm)[3], float& gcw) {
  for (int k = 0; k < 3; ++k) gm[k] = (pre[k] >= 0.f && pre[k] <= 1.f) ? g[k] : 0.f;
  gcw = g_cw - bg * (gm[0] + gm[1] + gm[2]);
}

struct MarchChunk { float a, w, T, gw, v[3], sw; };

// backward, one chunk (the last sample first): stores the lane's g_rgb, advances the running sum `back`, returns the lane's g_alpha
template <bool FUSED>
__device__ __forceinline__ float march_bwd_chunk(const MarchChunk& ck, const int c0, const int lane, const bool live, const int stop,
                                                 const bool has_rgb, const bool has_sw, const float (&gm)[3], const float gcw,
                                                 const float gd, float& back, float* __restrict__ g_rgb) {
  const int i = c0 + lane;
  const float a = ck.a, w = ck.w, T = ck.T;
  float gw = ck.gw;
  if (FUSED && live) {
    float wr = 0.f;
    if (has_rgb) for (int k = 0; k < 3; ++k) { wr += gm[k] * ck.v[k]; if (g_rgb) g_rgb[i * 3 + k] = w * gm[k]; }
    gw += wr + gcw + (has_sw ? gd * ck.sw : 0.f);
  }
  int hi = stop - c0;           // samples [c0, stop) of this chunk take part
  if (hi > 64) hi = 64;
  // the running sum `back` is sequential (fp32, last sample first); everything else of a sample's gradient - the double-precision
  // division included - only needs the value `back` had when the sequence reached it: the serial loop is one add per sample and
  // hands lane j its value, the rest is evaluated by all lanes at once (same operations per sample, same results)
  const float gww = gw * w;
  float myback = 0.f;
  for (int j = hi - 1; j >= 0; --j) {
    if (lane == j) myback = back;
    back += lane_value(gww, j);
  }
  float ga = 0.f;
  if (lane < hi) {
    const float gwT = gw * T;
    const double denom = (double)(1.f - a) + 1e-10;
    ga = (float)((double)gwT - (double)myback / denom);
  }
  return ga;
}

template <bool FUSED, bool DVGO>
__global__ __launch_bounds__(256) void k_march_fwd(const float* __restrict__ alpha, const float* __restrict__ rgb,
                                                   const float* __restrict__ step_w, const float* __restrict__ nrm_in,
                                                   const int32_t* __restrict__ ray_start, int n_rays, float bg,
                                                   float* __restrict__ weights, float* __restrict__ Tout,
                                                   float* __restrict__ alphainv_last, int32_t* __restrict__ i_end,
                                                   float* __restrict__ rgb_marched, float* __restrict__ rgb_pre,
                                                   float* __restrict__ cum_weights, float* __restrict__ depth_acc,
                                                   float* __restrict__ normal_marched) {
  const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave-uniform: the loop control below is scalar
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int b = ray_start[r], e = ray_start[r + 1];
  MarchAcc s;
  s.stop = e;
  float a_next = (b + lane < e) ? alpha[b + lane] : 0.f;
  for (int c0 = b; c0 < e; c0 += 64) {
    int i = c0 + lane;
    const float a = a_next;
    // everything the chunk needs from memory is requested before the sequential loop (and the next chunk's alpha with it): the
    // loop is ~100 ns per sample of pure latency, the loads land underneath it
    a_next = (i + 64 < e) ? alpha[i + 64] : 0.f;
    float cr[3] = {0.f, 0.f, 0.f}, cs = 0.f, cn[3] = {0.f, 0.f, 0.f};
    if (FUSED && i < e) {
      if (rgb) for (int k = 0; k < 3; ++k) cr[k] = rgb[i * 3 + k];
      if (step_w) cs = step_w[i];
      if (nrm_in) for (int k = 0; k < 3; ++k) cn[k] = nrm_in[i * 3 + k];
    }
    float myT, myw;
    march_fwd_chunk<FUSED, DVGO>(s, c0, e, lane, a, rgb != nullptr, cr, step_w != nullptr, cs, nrm_in != nullptr, cn, myT, myw);
    if (i < e) {
      weights[i] = myw;
      if (Tout) Tout[i] = myT;
    }
  }
  float pre[3], rgbm[3];
  march_fwd_finish<FUSED>(s, r, lane, bg, alphainv_last, i_end, rgb_marched, rgb_pre, cum_weights, depth_acc, normal_marched, pre,
                          rgbm);
}

template <bool FUSED>
__global__ __launch_bounds__(256) void k_march_bwd(const float* __restrict__ alpha, const float* __restrict__ rgb,
                                                   const float* __restrict__ step_w, const float* __restrict__ weights,
                                                   const float* __restrict__ Tin, const float* __restrict__ alphainv_last,
                                                   const int32_t* __restrict__ ray_start, const int32_t* __restrict__ i_end,
                                                   int n_rays, float bg, const float* __restrict__ rgb_pre,
                                                   const float* __restrict__ g_rgbm, const float* __restrict__ g_cw,
                                                   const float* __restrict__ g_last, const float* __restrict__ g_depth,
                                                   const float* __restrict__ g_w_in, float* __restrict__ g_alpha,
                                                   float* __restrict__ g_rgb) {
  const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (r >= n_rays) return;
  const int b = ray_start[r], e = ray_start[r + 1], stop = i_end[r];
  float gm[3] = {0, 0, 0}, gcw = 0.f, gd = 0.f;
  if (FUSED) {
    float pre[3], g[3];
    for (int k = 0; k < 3; ++k) {
      pre[k] = rgb_pre ? rgb_pre[r * 3 + k] : 0.5f;
      g[k] = g_rgbm ? g_rgbm[r * 3 + k] : 0.f;
    }
    march_bwd_ray(pre, g, g_cw ? g_cw[r] : 0.f, bg, gm, gcw);
    gd = g_depth ? g_depth[r] : 0.f;
  }
  float back = (g_last ? g_last[r] : 0.f) * alphainv_last[r];
  int nchunk = (e - b + 63) / 64;
  // a chunk's operands are requested one chunk ahead, so that they land under the sequential loop of the chunk before
  auto fetch = [&](int c) {
    MarchChunk k;
    const int i = b + c * 64 + lane;
    const bool live = i < e;
    k.a = live ? alpha[i] : 0.f;
    k.w = live ? weights[i] : 0.f;
    k.T = live ? Tin[i] : 1.f;
    k.gw = (live && g_w_in) ? g_w_in[i] : 0.f;
    k.v[0] = k.v[1] = k.v[2] = 0.f; k.sw = 0.f;
    if (FUSED && live) {
      if (rgb) for (int q = 0; q < 3; ++q) k.v[q] = rgb[i * 3 + q];
      if (step_w) k.sw = step_w[i];
    }
    return k;
  };
  MarchChunk nx = fetch(nchunk > 0 ? nchunk - 1 : 0);
  for (int c = nchunk - 1; c >= 0; --c) {
    int c0 = b + c * 64;
    int i = c0 + lane;
    bool live = i < e;
    const MarchChunk ck = nx;
    if (c > 0) nx = fetch(c - 1);
    const float ga = march_bwd_chunk<FUSED>(ck, c0, lane, live, stop, rgb != nullptr, step_w != nullptr, gm, gcw, gd, back, g_rgb);
    if (live) g_alpha[i] = ga;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Composite, ray losses and compositing backward of a ray by ONE wavefront in ONE launch: the steps above and the
// per-ray expressions of k_loss_rays (pp_loss_body.h) in sequence, for rays of at most 64 * MLB_CHUNKS samples.  What the
// backward needs of the forward - alpha, weight, transmittance, colour, step weight of every sample - stays in REGISTERS, one
// set per chunk (the chunk loops are unrolled): nothing the wavefront has stored is read back through a __restrict__ pointer.
// Every output of the three kernels is written; all but the four loss values are bit-identical to the separate launches.
// Loss values: a work-group's three sums go to its row of `work` by returning agent-scope atomics, one lane waits for them and
// draws a ticket (returning as well, no fence); the work-group that draws the last one reads all rows by agent-scope atomic loads,
// adds them in a fixed order (thread t: rows t, t + 256, ...; then the tree of block_sum256), adds the result to loss_out and
// leaves the ticket zero.  No work-group waits for another.
// work: [0] ticket | [4 + 4 * g .. + 3) row of work-group g
// ------------------------------------------------------------------------------------------------------------------
#define MLB_CHUNKS 3
__global__ __launch_bounds__(256) void k_march_loss_bwd(
    const float* __restrict__ alpha, const float* __restrict__ rgb, const float* __restrict__ step_w,
    const int32_t* __restrict__ ray_start, int n_rays, float bg, float* __restrict__ weights, float* __restrict__ Tout,
    float* __restrict__ alphainv_last, int32_t* __restrict__ i_end, float* __restrict__ rgb_marched, float* __restrict__ rgb_pre,
    float* __restrict__ cum_weights, float* __restrict__ depth_acc, const float* __restrict__ target,
    const float* __restrict__ mask_px, float* __restrict__ mask_sum, float w_main, float w_ent, float w_mask, float ls,
    float* __restrict__ g_rgbm, float* __restrict__ g_last, float* __restrict__ g_cw, float* __restrict__ loss_out,
    const float* __restrict__ g_depth, const float* __restrict__ g_w_in, float* __restrict__ g_alpha, float* __restrict__ g_rgb,
    float* work) {
  __shared__ float sm[4];
  __shared__ float s_loss[4][3];
  __shared__ int s_last;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = blockIdx.x * 4 + wid;
  const int lane = threadIdx.x & 63;
  const float msum = loss_mask_sum(mask_px, n_rays, sm);         // k_loss_rays' own sum, in its order: the same bits in every work-group
  if (blockIdx.x == 0 && threadIdx.x == 0) mask_sum[0] = msum;
  const float invN = 1.f / (float)n_rays;
  float l_mse = 0.f, l_ent = 0.f, l_bce = 0.f;
  if (r < n_rays) {
    const int b = ray_start[r];
    int e = ray_start[r + 1];
    if (e - b > 64 * MLB_CHUNKS) e = b + 64 * MLB_CHUNKS;        // the caller promised it is not (sample_cap); never index past the registers
    const int nchunk = (e - b + 63) / 64;
    // ---- (a) forward
    MarchAcc s;
    s.stop = e;
    float ka[MLB_CHUNKS], kw[MLB_CHUNKS], kT[MLB_CHUNKS], kr[MLB_CHUNKS][3], ks[MLB_CHUNKS];
    const float no3[3] = {0.f, 0.f, 0.f};
    float a_next = (b + lane < e) ? alpha[b + lane] : 0.f;
#pragma unroll
    for (int c = 0; c < MLB_CHUNKS; ++c) {
      ka[c] = 0.f; kw[c] = 0.f; kT[c] = 1.f; ks[c] = 0.f;
      for (int k = 0; k < 3; ++k) kr[c][k] = 0.f;
      if (c < nchunk) {
        const int c0 = b + c * 64, i = c0 + lane;
        ka[c] = a_next;
        a_next = (i + 64 < e) ? alpha[i + 64] : 0.f;
        if (i < e) {
          for (int k = 0; k < 3; ++k) kr[c][k] = rgb[i * 3 + k];
          if (step_w) ks[c] = step_w[i];
        }
        march_fwd_chunk<true, false>(s, c0, e, lane, ka[c], true, kr[c], step_w != nullptr, ks[c], false, no3, kT[c], kw[c]);
        if (i < e) {
          weights[i] = kw[c];
          Tout[i] = kT[c];
        }
      }
    }
    float pre[3], rgbm[3];
    march_fwd_finish<true>(s, r, lane, bg, alphainv_last, i_end, rgb_marched, rgb_pre, cum_weights, depth_acc, nullptr, pre, rgbm);
    // ---- (b) the ray's loss terms and the gradients of its render outputs (wave-uniform: every lane holds the ray's sums)
    const float tgt[3] = {target[r * 3], target[r * 3 + 1], target[r * 3 + 2]};
    const RayLoss L = loss_ray_terms(rgbm, s.Tc, s.w, tgt, mask_px[r], msum, invN, w_main, w_ent, w_mask, ls);
    l_mse = L.l_mse; l_ent = L.l_ent; l_bce = L.l_bce;
    if (lane == 0) {
      for (int k = 0; k < 3; ++k) g_rgbm[r * 3 + k] = L.g_rgbm[k];
      g_last[r] = L.g_last;
      g_cw[r] = L.g_cw;
    }
    // ---- (c) backward
    float gm[3], gcw;
    march_bwd_ray(pre, L.g_rgbm, L.g_cw, bg, gm, gcw);
    const float gd = g_depth ? g_depth[r] : 0.f;
    float back = L.g_last * s.Tc;
    float kg[MLB_CHUNKS];
#pragma unroll
    for (int c = 0; c < MLB_CHUNKS; ++c) {
      const int i = b + c * 64 + lane;
      kg[c] = (g_w_in && c < nchunk && i < e) ? g_w_in[i] : 0.f;
    }
#pragma unroll
    for (int c = MLB_CHUNKS - 1; c >= 0; --c) {
      if (c < nchunk) {
        const int c0 = b + c * 64, i = c0 + lane;
        const bool live = i < e;
        MarchChunk ck;
        ck.a = ka[c]; ck.w = kw[c]; ck.T = kT[c]; ck.gw = kg[c]; ck.sw = ks[c];
        for (int k = 0; k < 3; ++k) ck.v[k] = kr[c][k];
        const float ga = march_bwd_chunk<true>(ck, c0, lane, live, s.stop, true, step_w != nullptr, gm, gcw, gd, back, g_rgb);
        if (live) g_alpha[i] = ga;
      }
    }
  }
  // ---- (d) loss values
  if (lane == 0) { s_loss[wid][0] = l_mse; s_loss[wid][1] = l_ent; s_loss[wid][2] = l_bce; }
  __syncthreads();
  unsigned* ticket = reinterpret_cast<unsigned*>(work);
  float* rows = work + 4;
  if (threadIdx.x == 0) {
    for (int k = 0; k < 3; ++k) {
      const float v = ((s_loss[0][k] + s_loss[1][k]) + s_loss[2][k]) + s_loss[3][k];
      const float old = __hip_atomic_exchange(rows + blockIdx.x * 4 + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("" ::"v"(old));               // the returned value is "used": the returning form stays
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the row is in place before the arrival is counted
    s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  float t[3] = {0.f, 0.f, 0.f};
  for (int g = threadIdx.x; g < (int)gridDim.x; g += 256)
    for (int k = 0; k < 3; ++k) t[k] += __hip_atomic_load(rows + g * 4 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int k = 0; k < 3; ++k) t[k] = block_sum256(t[k], sm);
  if (threadIdx.x == 0) {
    if (loss_out) loss_rays_add(loss_out, t[0], t[1], t[2], msum, invN, w_main, w_ent, w_mask);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

extern "C" int pp_alpha2weight_fwd(const float* alpha, const int32_t* ray_start, int32_t n_rays, float* weights,
                                   float* T, float* alphainv_last, int32_t* i_end, void* stream) {
  PP_REQUIRE(alpha && ray_start && weights && T && alphainv_last && i_end, "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  hipLaunchKernelGGL((k_march_fwd<false, false>), dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, nullptr,
                     nullptr, nullptr, ray_start, n_rays, 0.f, weights, T, alphainv_last, i_end, nullptr, nullptr,
                     nullptr, nullptr, nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_alpha2weight_bwd(const float* alpha, const float* weights, const float* T, const float* alphainv_last,
                                   const int32_t* ray_start, const int32_t* i_end, int32_t n_rays,
                                   const float* grad_weights, const float* grad_last, float* grad_alpha, void* stream) {
  PP_REQUIRE(alpha && weights && T && alphainv_last && ray_start && i_end && grad_weights && grad_last && grad_alpha,
             "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  hipLaunchKernelGGL((k_march_bwd<false>), dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, nullptr,
                     nullptr, weights, T, alphainv_last, ray_start, i_end, n_rays, 0.f, nullptr, nullptr, nullptr,
                     grad_last, nullptr, grad_weights, grad_alpha, nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_march_fwd(const float* alpha, const float* rgb, const float* step_w, const float* nrm_in,
                            const int32_t* ray_start, int32_t n_rays, float bg, float* weights, float* T,
                            float* alphainv_last, int32_t* i_end, float* rgb_marched, float* rgb_pre,
                            float* cum_weights, float* depth_acc, float* normal_marched, void* stream) {
  PP_REQUIRE(alpha && rgb && ray_start && weights && T && alphainv_last && i_end && cum_weights, "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  hipLaunchKernelGGL((k_march_fwd<true, false>), dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, rgb,
                     step_w, nrm_in, ray_start, n_rays, bg, weights, T, alphainv_last, i_end, rgb_marched, rgb_pre,
                     cum_weights, depth_acc, normal_marched);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_march_bwd(const float* alpha, const float* rgb, const float* step_w, const float* weights,
                            const float* T, const float* alphainv_last, const int32_t* ray_start,
                            const int32_t* i_end, int32_t n_rays, float bg, const float* rgb_pre,
                            const float* g_rgb_marched, const float* g_cum_weights, const float* g_alphainv_last,
                            const float* g_depth_acc, const float* g_weights, float* grad_alpha, float* grad_rgb,
                            void* stream) {
  PP_REQUIRE(alpha && rgb && weights && T && alphainv_last && ray_start && i_end && grad_alpha, "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  hipLaunchKernelGGL((k_march_bwd<true>), dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, rgb,
                     step_w, weights, T, alphainv_last, ray_start, i_end, n_rays, bg, rgb_pre, g_rgb_marched,
                     g_cum_weights, g_alphainv_last, g_depth_acc, g_weights, grad_alpha, grad_rgb);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_march_loss_workspace(int32_t n_rays, int32_t sample_cap, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  PP_REQUIRE(sample_cap > 0 && sample_cap <= 64 * MLB_CHUNKS, "sample_cap: the kernel holds at most 192 samples of a ray");
  *bytes = (int64_t)(4 + 4 * pp_div_up(n_rays, 4)) * sizeof(float);
  return PP_OK;
}

extern "C" int pp_march_loss_bwd(const float* alpha, const float* rgb, const float* step_w, const int32_t* ray_start,
                                 int32_t n_rays, int32_t sample_cap, float bg, float* weights, float* T, float* alphainv_last,
                                 int32_t* i_end, float* rgb_marched, float* rgb_pre, float* cum_weights, float* depth_acc,
                                 const float* target, const float* mask_px, float* mask_sum, float w_main, float w_entropy,
                                 float w_mask, float loss_scale, float* g_rgb_marched, float* g_alphainv_last,
                                 float* g_cum_weights, float* loss_out, const float* g_depth_acc, const float* g_weights,
                                 float* grad_alpha, float* grad_rgb, void* work, int64_t work_bytes, void* stream) {
  PP_REQUIRE(alpha && rgb && ray_start && weights && T && alphainv_last && i_end && rgb_marched && rgb_pre && cum_weights,
             "null pointer (compositing)");
  PP_REQUIRE(target && mask_px && mask_sum && g_rgb_marched && g_alphainv_last && g_cum_weights, "null pointer (losses)");
  PP_REQUIRE(grad_alpha && work, "null pointer (backward / workspace)");
  int64_t need = 0;
  if (int st = pp_march_loss_workspace(n_rays, sample_cap, &need)) return st;
  PP_REQUIRE(work_bytes >= need && (reinterpret_cast<uintptr_t>(work) & 15) == 0, "workspace too small or not 16-byte aligned");
  hipLaunchKernelGGL(k_march_loss_bwd, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, rgb, step_w, ray_start,
                     n_rays, bg, weights, T, alphainv_last, i_end, rgb_marched, rgb_pre, cum_weights, depth_acc, target, mask_px,
                     mask_sum, w_main, w_entropy, w_mask, loss_scale, g_rgb_marched, g_alphainv_last, g_cum_weights, loss_out,
                     g_depth_acc, g_weights, grad_alpha, grad_rgb, static_cast<float*>(work));
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Surface-point query: first sign change of the SDF along a ray + linear zero crossing
// (Voxurf.query_sdf_point_wocuda / _wodeform, lib/voxurf_coarse.py:766-795, :809-837).  One wavefront per ray.
// Compact mode (ray_start != NULL): sdf[M] holds the in-bbox samples, the dense row is rebuilt with the reference's
// default value 1 for out-of-bbox slots (:752).  Dense mode: sdf is already [N,S].
// ------------------------------------------------------------------------------------------------------------------
#define PP_MAX_S 1024
__global__ __launch_bounds__(256) void k_first_crossing(const float* __restrict__ sdf, const int32_t* __restrict__ ray_start,
                                                        const int32_t* __restrict__ step_k, int n_rays, int S, float dist,
                                                        const float* __restrict__ t_min, const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, float* __restrict__ sdf_dense,
                                                        float* __restrict__ pts, uint8_t* __restrict__ mask,
                                                        float* __restrict__ zval) {
  __shared__ float rows[4][PP_MAX_S];
  int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int r = blockIdx.x * 4 + wid;
  if (r >= n_rays) return;
  float* row = rows[wid];
  if (ray_start) {
    for (int k = lane; k < S; k += 64) row[k] = 1.f;
    __builtin_amdgcn_wave_barrier();
    for (int i = ray_start[r] + lane; i < ray_start[r + 1]; i += 64) row[step_k[i]] = sdf[i];
  } else {
    for (int k = lane; k < S; k += 64) row[k] = sdf[(size_t)r * S + k];
  }
  __builtin_amdgcn_wave_barrier();
  if (sdf_dense) for (int k = lane; k < S; k += 64) sdf_dense[(size_t)r * S + k] = row[k];
  int prev = 0;                                        // argmax of an all-zero row is 0 (voxurf_coarse.py:771)
  for (int k0 = 0; k0 < S - 1; k0 += 64) {
    int k = k0 + lane;
    bool hit = (k < S - 1) && (row[k] * row[k + 1] <= 0.f);
    unsigned long long bal = __ballot(hit);
    if (bal) { prev = k0 + __ffsll((long long)bal) - 1; break; }
  }
  if (lane == 0) {
    float s1 = row[prev], s2 = row[prev + 1];
    float z1 = (float)prev * dist + dist * 0.5f, z2 = (float)(prev + 1) * dist + dist * 0.5f;
    float z0 = (s1 * z2 - s2 * z1) / (s1 - s2 + 1e-10f);
    if (z0 < z1) z0 = 0.f;
    if (z0 > z2) z0 = 0.f;
    bool ok = (z0 > 1e-10f) && (s1 * s2 < 0.f);
    float dx = rays_d[r * 3], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
    float nrm = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
    float interpx = t_min[r] + z0 / nrm;
    pts[r * 3] = rays_o[r * 3] + dx * interpx;
    pts[r * 3 + 1] = rays_o[r * 3 + 1] + dy * interpx;
    pts[r * 3 + 2] = rays_o[r * 3 + 2] + dz * interpx;
    mask[r] = ok ? 1 : 0;
    if (zval) zval[r] = z0;
  }
}

extern "C" int pp_sdf_first_crossing(const float* sdf, const int32_t* ray_start, const int32_t* step_k, int32_t n_rays,
                                     int32_t n_samples, float dist, const float* t_min, const float* rays_o,
                                     const float* rays_d, float* sdf_dense, float* pts, uint8_t* mask, float* zval,
                                     void* stream) {
  PP_REQUIRE(sdf && t_min && rays_o && rays_d && pts && mask, "null pointer");
  PP_REQUIRE((ray_start == nullptr) == (step_k == nullptr), "ray_start and step_k go together");
  PP_REQUIRE(n_rays > 0 && n_samples >= 2 && n_samples <= PP_MAX_S, "need n_rays>0 and 2<=n_samples<=1024");
  hipLaunchKernelGGL(k_first_crossing, dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), sdf, ray_start, step_k,
                     n_rays, n_samples, dist, t_min, rays_o, rays_d, sdf_dense, pts, mask, zval);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// DirectVoxGO compositing (lib/dvgo_ori.py:478-489, :361-366): exclusive cumprod of clamp_min(1-alpha, 1e-10) without
// early termination; rgb_marched = sum w*rgb + alphainv_last*bg (clamped), depth_acc = sum w*step_w.
extern "C" int pp_march_dvgo_fwd(const float* alpha, const float* rgb, const float* step_w, const int32_t* ray_start,
                                 int32_t n_rays, float* weights, float* T, float* alphainv_last, int32_t* i_end,
                                 float* rgb_acc, float* cum_weights, float* depth_acc, void* stream) {
  PP_REQUIRE(alpha && ray_start && weights && T && alphainv_last && i_end && cum_weights, "null pointer");
  PP_REQUIRE(n_rays > 0, "n_rays<=0");
  hipLaunchKernelGGL((k_march_fwd<true, true>), dim3(pp_div_up(n_rays, 4)), dim3(256), 0, pp_stream(stream), alpha, rgb,
                     step_w, nullptr, ray_start, n_rays, 0.f, weights, T, alphainv_last, i_end, nullptr, rgb_acc,
                     cum_weights, depth_acc, nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
