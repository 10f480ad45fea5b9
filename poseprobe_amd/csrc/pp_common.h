// Shared device/host helpers for libposeprobe_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/poseprobe_hip.h"

#define PP_WAVE 64

void pp_set_error(const char* fmt, ...);

// Options (include/poseprobe_hip.h: pp_context_set_option / pp_context_get_option).  They are fields of a caller-owned
// pp_context that travels with every call whose behaviour they select; a NULL context means the compiled-in defaults.
// An entry point reads them once, from the context it was handed (pp_options), and passes what it resolved down to its launch
// helpers as arguments.  The library holds NO process-wide mutable state, no per-thread state beside the error text, and never
// reads the environment.
enum PPOption {
  PP_OPT_MLP_FUSED = 0,        // 1: layer-fused object-branch MLP kernels, 0: layer-by-layer GEMMs (A/B runs)
  PP_OPT_GRID_CHUNKS,          // x-chunks of the fused TV + Adam pass (0 = heuristic)
  PP_OPT_NERF_SPLIT,           // scene branch: every matrix product as three fp16 products (1) or on the fp32 instructions (0)
  PP_OPT_MLP_SPLIT,            // bit mask: layer-fused object-branch MLP kernels with three fp16 products per fp32 product (pp_mlp_split.hip); 1 warp fwd, 2 warp bwd, 4 rgb fwd, 8 rgb bwd, 16 weight-gradient chains
  PP_OPT_MLP_WGS,              // work-groups of the persistent object-branch MLP kernels (0 = one per CU); fewer leave CUs to a concurrent HBM-bound kernel
  PP_OPT_NERF_CHAIN,           // scene branch: 3 = the fused route: the eight feature layers, the density head and the colour head's hidden layer of the forward pass as one
                               // kernel with the tile resident in LDS (pp_nerf_trunk.h), the data-gradient chain of the backward pass as one more; 0 = one GEMM per layer
                               // (the tests' reference).  1 and 2, a retired hybrid of the two, are refused
  PP_OPT_MLP_PACK,             // 1: the split-precision object-branch MLP kernels read a weight pack recorded in the context by pp_mlp_pack
                               // for the params pointer they are given, 0: they always derive it in their prologues
  PP_OPT_WARP_LEAN,            // 1: pp_warp_lean_begin records a lean scope (the warp net's kernels then leave out what the weight-gradient
                               // kernel can rebuild), 0: it records nothing - every call takes the full form (A/B runs)
  PP_OPT_COUNT
};

// Caller-owned context: the option values + five records (weight pack, lean scope, the two ordered-flush workspaces, join scope).  It owns no HIP
// object: every kernel runs on the stream the call is given.
struct PPContext {
  int opt[PP_OPT_COUNT];
  // weight pack of the object-branch MLPs (pp_mlp_pack): the buffer and the two parameter blocks it was computed from
  // ([0] warp net, [1] rgbnet); pack == nullptr: none
  const float* pack;
  const float* pack_params[2];
  // lean scope of the warp net (pp_warp_lean_begin): the buffers and the parameter block it was opened for; lean_acts == nullptr: none
  const float* lean_acts;
  const float* lean_scratch;
  const float* lean_params;
  // workspace of the ordered gradient flushes (pp_ordered_attach, pp_ordered.h) and the sizes it was attached for;
  // ord == nullptr: none, every flush uses float atomics
  float* ord;
  int ord_wgs, ord_cap, ord_rays;
  // workspace of the scene branch's ordered weight-gradient flush (pp_nerf_ordered_attach, pp_gemm_tn_tr.h);
  // nerf_ord == nullptr: none, pp_nerf_bwd flushes with float atomics
  float* nerf_ord;
  // join scope of the weight gradients (pp_wgrad_join_begin): open or not, and the rgbnet chain that a pp_rgbnet_bwd inside it
  // left to the next warp chain on this context (the arguments of its launch); join_pending == false: none
  bool join_open, join_pending;
  struct {
    const float *feat, *acts, *scratch;
    const int32_t* count;
    int capacity;
    float* params_grad;
    hipStream_t stream;
  } join;
};

// The option array of a context (indexed by PPOption), or the compiled-in defaults for ctx == nullptr.  Two contexts with
// different arithmetic coexist in one process, also on different threads at the same time.
const int* pp_options(const void* ctx);
int pp_num_cus();                                           // compute units of the current device (queried once per process: a hardware constant)
// X-marching total-variation value / gradient pass on a channels-last grid (pp_optim.hip); false: shape not covered
bool pp_launch_tv_march(const float* p, int X, int Y, int Z, int C, float scale, const float* g_scalar, float* grad, float* tv_out,
                        hipStream_t st);

#define PP_REQUIRE(cond, msg)                                     \
  do {                                                            \
    if (!(cond)) {                                                \
      pp_set_error("%s: %s", __func__, msg);                      \
      return PP_ERR_INVALID_ARG;                                  \
    }                                                             \
  } while (0)

#define PP_CHECK_LAUNCH()                                                           \
  do {                                                                              \
    hipError_t e__ = hipGetLastError();                                             \
    if (e__ != hipSuccess) {                                                        \
      pp_set_error("%s: kernel launch failed: %s", __func__, hipGetErrorString(e__)); \
      return PP_ERR_LAUNCH;                                                         \
    }                                                                               \
  } while (0)

static inline hipStream_t pp_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int pp_div_up(int a, int b) { return (a + b - 1) / b; }

// Scene constants passed by value to kernels (kernarg), derived once on the host.
struct SceneDev {
  float mn[3], mx[3];
  int sz[3];
  float voxel, stepsize, near_, far_, bg;
  int S;
  float out_range;
  int C, Lp, Lv;
  int flat_f32;   // custom SDF sampler: form the flat voxel index in fp32 as the reference does (only differs above 2^24 voxels)
};

static inline SceneDev pp_scene_dev(const pp_scene* s) {
  SceneDev d;
  for (int i = 0; i < 3; ++i) { d.mn[i] = s->xyz_min[i]; d.mx[i] = s->xyz_max[i]; d.sz[i] = s->size[i]; }
  d.voxel = s->voxel_size; d.stepsize = s->stepsize; d.near_ = s->near_clip; d.far_ = s->far_clip; d.bg = s->bg;
  d.S = s->n_samples; d.out_range = s->out_range; d.C = s->k0_dim; d.Lp = s->pos_pe; d.Lv = s->view_pe;
  // lib/voxurf_coarse.py:632-647 computes `iz * IW * IH + iy * IW + ix` on FLOAT tensors before .long(): beyond 2^24 voxels
  // (grids above 256^3) odd flat indices are not representable and round to a neighbouring voxel.  Reproduced by default
  // for parity (SURVEY 8a parity hazards); pp_scene.sdf_index_exact = 1 gives the exact index.
  d.flat_f32 = ((long long)s->size[0] * s->size[1] * s->size[2] > (1ll << 24)) && s->sdf_index_exact == 0;
  return d;
}

#ifdef __HIPCC__
// exact-rounding primitives: the library is built with -ffp-contract=off, these document intent where the
// op order of the reference must be reproduced bit for bit (sampler / coordinate transforms).
__device__ __forceinline__ float pp_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float pp_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float pp_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float pp_div(float a, float b) { return __fdiv_rn(a, b); }

__device__ __forceinline__ float pp_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// softplus(beta=10, threshold=20) as torch.nn.Softplus
__device__ __forceinline__ float pp_softplus10(float x) {
  float bx = 10.0f * x;
  return bx > 20.0f ? x : log1pf(expf(bx)) / 10.0f;
}
__device__ __forceinline__ float pp_dsoftplus10(float x) {
  float bx = 10.0f * x;
  return bx > 20.0f ? 1.0f : pp_sigmoid(bx);
}

__device__ __forceinline__ float pp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// world -> continuous voxel coordinate along one axis, op order of grid_sampler + grid_sample_3d
// (lib/voxurf_coarse.py:528, :553-555): t=(p-min)/(max-min); n=t*2-1; u=((n+1)/2)*(size-1)
__device__ __forceinline__ float pp_grid_u(float p, float mn, float mx, int size) {
  float t = pp_div(pp_sub(p, mn), pp_sub(mx, mn));
  float n = pp_sub(pp_mul(t, 2.0f), 1.0f);
  return pp_mul(pp_div(pp_add(n, 1.0f), 2.0f), (float)(size - 1));
}
#endif
