// The two shallow MLPs of the object branch on the CDNA4 matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32).
//
//  * rgbnet  64(57)->128->128->128->3 + sigmoid            (lib/voxurf_coarse.py:208-216, :1032-1033)
//  * warp    3->128->128->128->128->4, ReLU                 (lib/deformation/deform_net.py:12-31, modules.py:43-124)
//
// The warp net is evaluated in "4-row" form: for every sample row 0 is the primal activation and rows 1-3 are the
// forward-mode tangents d/dp_i.  A hidden layer is then ONE GEMM over 4M rows whose epilogue adds the bias to row 0
// only and applies row 0's ReLU mask to all four rows; the backward of (value + Jacobian) is the same GEMM chain
// run in reverse with identical masking.  This replaces the reference's four autograd.grad(create_graph=True)
// passes and their double backward (lib/voxurf_coarse.py:968-984) by plain matrix products.
//
// This file holds the C-ABI entry points of both MLPs: argument checks, the records a context carries for them (weight pack, lean
// scope, ordered-flush workspace, join scope of the weight gradients) and the routing of a call to its kernels, decided once per call (MlpRoute).  The kernels are
// elsewhere: layer-fused on the fp32 matrix instructions in pp_mlp_fused.hip, layer-fused split-precision in pp_mlp_split.hip,
// layer by layer (generic MLP shapes, option mlp_fused = 0) in pp_mlp_layered.hip.
#include "pp_common.h"
#include "pp_mlp_fused.h"
#include "pp_mlp_pack.h"
#include "pp_ordered.h"
#include <stdlib.h>

// What one call runs, resolved once at the top of its entry point from the context it is handed (nullptr: the compiled-in defaults).
// The helpers below take the route: none of them reads an option itself.
struct MlpRoute {
  const PPContext* c;    // the records: weight pack, lean scope, ordered-flush workspace; nullptr: no context
  bool fused;            // option mlp_fused: the layer-fused kernels run (0: layer by layer, as generic MLP shapes always do)
  int split;             // option mlp_split: which of the layer-fused kernels are the split-precision ones (bits: enum PPOption)
  bool pack;             // option mlp_pack: the split-precision kernels may read a recorded weight pack
  // persistent grid of the fused kernels: one work-group per CU (weights stationary in ~200 registers per lane, LDS 70-156 KB;
  // 256 on an MI355X in SPX mode), or option mlp_wgs - at least 16: the weight-gradient chains share them out over three layers
  int wgs;
  explicit MlpRoute(const void* ctx) : c(static_cast<const PPContext*>(ctx)) {
    const int* o = pp_options(ctx);
    fused = o[PP_OPT_MLP_FUSED] == 1; split = o[PP_OPT_MLP_SPLIT]; pack = o[PP_OPT_MLP_PACK] == 1;
    wgs = o[PP_OPT_MLP_WGS] > 0 ? (o[PP_OPT_MLP_WGS] < 16 ? 16 : o[PP_OPT_MLP_WGS]) : pp_num_cus();
  }
  // this call runs the split-precision layer-fused kernels `bits` (all of them)
  bool runs_split(int bits) const { return fused && (split & bits) == bits; }
};

// the weight pack a split-precision kernel may read instead of its prologue: only the one recorded in THIS call's context for
// exactly these params (net 0: warp net, 1: rgbnet); no context, option mlp_pack = 0 or another pointer: none
static const float* mlp_pack_for(const MlpRoute& rt, const float* params, int net) {
  if (!rt.c || !rt.pack || !rt.c->pack || rt.c->pack_params[net] != params) return nullptr;
  return rt.c->pack;
}

// Lean scope of the warp net (pp_warp_lean_begin): a call takes the lean form only with the context that holds the record, for
// exactly the recorded buffers (scratch == nullptr: the forward pass, which has none) and while all three kernels are the
// split-precision ones - the other paths cannot honour a lean image.  Returns the recorded params pointer (the block the scope's
// calls are made with: the weight-gradient stage, which is not handed one, reads W0 and W4 from it), or nullptr = full form.
static const float* warp_lean_for(const MlpRoute& rt, const float* acts, const float* scratch) {
  const PPContext* c = rt.c;
  if (!c || !c->lean_acts || c->lean_acts != acts || (scratch && c->lean_scratch != scratch) || !rt.runs_split(1 | 2 | 16)) return nullptr;
  return c->lean_params;
}

extern "C" int pp_warp_lean_end(void* ctx) {
  PP_REQUIRE(ctx, "null context");
  PPContext* c = static_cast<PPContext*>(ctx);
  c->lean_acts = c->lean_scratch = c->lean_params = nullptr;
  return PP_OK;
}

extern "C" int pp_warp_lean_begin(const float* acts, const float* scratch, const float* params, void* ctx) {
  PP_REQUIRE(ctx, "null context (the scope is recorded in a context: create one)");
  PP_REQUIRE(acts && scratch && params, "null pointer");
  pp_warp_lean_end(ctx);
  if (pp_options(ctx)[PP_OPT_WARP_LEAN] != 1 || !MlpRoute(ctx).runs_split(1 | 2 | 16)) return PP_OK;
  PPContext* c = static_cast<PPContext*>(ctx);
  c->lean_acts = acts;
  c->lean_scratch = scratch;
  c->lean_params = params;
  return PP_OK;
}

// Ordered flushes (pp_ordered_attach): with a workspace recorded in the call's context the parameter gradients of the backward
// chains are added up in a fixed order instead of by float atomics.  Only the split-precision layer-fused kernels have that
// path: everything else is refused while a workspace is attached rather than left on atomics.
// `bits`: the mlp_split bits of the kernels the call runs.  Returns the reason for a refusal, or nullptr.
static const char* ordered_refusal(const MlpRoute& rt, int capacity, int bits, bool fused_shape = true) {
  const PPContext* c = rt.c;
  if (!c || !c->ord) return nullptr;
  if (!fused_shape || !rt.runs_split(bits))
    return "an ordered-flush workspace is attached to the context: only the split-precision layer-fused kernels have ordered "
           "flushes (options mlp_fused = 1, mlp_split bits 2, 8 and 16; the Voxurf network shapes)";
  if (capacity > c->ord_cap || rt.wgs > c->ord_wgs)
    return "the attached ordered-flush workspace is too small for this capacity / work-group count";
  return nullptr;
}
#define PP_REQUIRE_ORDERED(rt, capacity, ...)                                   \
  do {                                                                          \
    const char* why__ = ordered_refusal(rt, capacity, __VA_ARGS__);             \
    PP_REQUIRE(why__ == nullptr, why__);                                        \
  } while (0)
// region of the attached workspace: 0 / 1 = weight-gradient chain of the warp net / rgbnet, 2 / 3 = their thin layers; nullptr: none
static float* ordered_part(const MlpRoute& rt, int region) {
  const PPContext* c = rt.c;
  if (!c || !c->ord) return nullptr;
  const OrdLayout L = pp_ord_layout(c->ord_wgs, c->ord_cap, c->ord_rays);
  return c->ord + (region < 2 ? L.wgrad[region] : L.thin[region - 2]);
}

extern "C" int pp_mlp_pack_workspace(int64_t* pack_floats) {
  PP_REQUIRE(pack_floats, "null pointer");
  *pack_floats = PK_FLOATS;
  return PP_OK;
}

extern "C" int pp_mlp_pack_invalidate(void* ctx) {
  PP_REQUIRE(ctx, "null context");
  PPContext* c = static_cast<PPContext*>(ctx);
  c->pack = nullptr;
  c->pack_params[0] = c->pack_params[1] = nullptr;
  return PP_OK;
}

extern "C" int pp_mlp_pack(const float* warp_params, const float* rgbnet_params, float* pack, void* ctx, void* stream) {
  PP_REQUIRE(ctx, "null context (the pack is recorded in a context: create one)");
  PP_REQUIRE(pack && (warp_params || rgbnet_params), "null pointer");
  PP_REQUIRE((reinterpret_cast<uintptr_t>(pack) & 15) == 0, "pack must be 16-byte aligned");
  pp_mlp_pack_invalidate(ctx);
  const MlpRoute rt(ctx);
  // nothing would read it: option off, or none of the four split-precision data-path kernels selected
  if (!rt.pack || !rt.fused || (rt.split & 15) == 0) return PP_OK;
  pp_launch_mlp_pack(warp_params, rgbnet_params, pack, pp_stream(stream));
  PP_CHECK_LAUNCH();
  PPContext* c = static_cast<PPContext*>(ctx);
  c->pack = pack;
  c->pack_params[0] = warp_params;
  c->pack_params[1] = rgbnet_params;
  return PP_OK;
}

// pp_pose_fwd, the upload of the step's scalars, the memset of the zero block and pp_mlp_pack in one launch (k_step_begin)
extern "C" int pp_step_begin(const float* se3, const float* w2c_init, const int32_t* refine_mask, int32_t n_views, float* w2c,
                             float* c2w, float* jac, const float* step_scalars, int32_t n_scalars, float* step_dev,
                             float* zero_block, int32_t n_zero, const float* warp_params, const float* rgbnet_params, float* pack,
                             void* ctx, void* stream) {
  PP_REQUIRE(se3 && w2c_init && w2c && c2w && jac && n_views > 0, "null pointer or n_views<=0");
  PP_REQUIRE(n_scalars >= 0 && n_scalars <= PP_STEP_SCALARS_MAX && (n_scalars == 0 || (step_scalars && step_dev)),
             "0 <= n_scalars <= 32, with step_scalars (host) and step_dev");
  PP_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero_block), "n_zero<0 or null zero_block");
  PP_REQUIRE(pack == nullptr || (ctx && (warp_params || rgbnet_params)), "a pack needs a context and parameters");
  PP_REQUIRE((reinterpret_cast<uintptr_t>(pack) & 15) == 0, "pack must be 16-byte aligned");
  PPStepScalars sv;
  sv.n = n_scalars;
  for (int i = 0; i < PP_STEP_SCALARS_MAX; ++i) sv.v[i] = i < n_scalars ? step_scalars[i] : 0.f;
  bool packs = false;
  if (ctx) {
    pp_mlp_pack_invalidate(ctx);
    const MlpRoute rt(ctx);
    packs = pack && rt.pack && rt.fused && (rt.split & 15) != 0;      // as pp_mlp_pack: otherwise nothing would read it
  }
  pp_launch_step_begin(se3, w2c_init, refine_mask, n_views, w2c, c2w, jac, sv, step_dev, zero_block, n_zero, warp_params,
                       rgbnet_params, packs ? pack : nullptr, pp_stream(stream));
  PP_CHECK_LAUNCH();
  if (packs) {
    PPContext* c = static_cast<PPContext*>(ctx);
    c->pack = pack;
    c->pack_params[0] = warp_params;
    c->pack_params[1] = rgbnet_params;
  }
  return PP_OK;
}

// Generic ReLU MLP  in_ld -> 128 -> ... -> 128 -> 3 (+ optional sigmoid), n_gemm = number of 128-wide hidden layers.
// Parameter block: W0[128*in_ld] b0[128] | (W[128*128] b[128]) x (n_gemm-1) | Wout[3*128] bout[3].
extern "C" int pp_mlp_fwd(const float* params, const float* feat, int32_t in_ld, int32_t n_gemm, const int32_t* count,
                          int32_t capacity, const float* logit_add, int32_t logit_add_ld, float* acts, float* out,
                          void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && feat && count && out, "null pointer");
  PP_REQUIRE(capacity > 0 && in_ld % 32 == 0 && in_ld <= 128 && n_gemm >= 1 && n_gemm <= 8, "bad sizes");
  // acts == NULL: forward only (no backward pass will follow: the activations are not written) - the split-precision fused kernel only
  PP_REQUIRE(acts || (in_ld == 64 && n_gemm == 3 && rt.runs_split(4)),
             "acts may be NULL only for the rgbnet shape with the split-precision forward kernel (option mlp_split bit 4)");
  hipStream_t st = pp_stream(stream);
  if (in_ld == 64 && n_gemm == 3 && rt.fused) {       // the Voxurf rgbnet shape: layer-fused kernel
    if (rt.runs_split(4)) pp_launch_rgb_fused_fwd_s(params, feat, count, capacity, logit_add, logit_add_ld, acts, out, st, rt.wgs, mlp_pack_for(rt, params, 1));
    else pp_launch_rgb_fused_fwd(params, feat, count, capacity, logit_add, logit_add_ld, acts, out, st, rt.wgs);
  } else
    pp_launch_mlp_layered_fwd(params, feat, in_ld, n_gemm, count, capacity, logit_add, logit_add_ld, acts, out, st);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------ fused backward, two stages
// Stage 1 of a layer-fused backward chain: the data-gradient kernel (split-precision or fp32 instructions), which also produces
// the thin layers' gradients and leaves Ybar of the hidden layers in `scratch`.  Returns whether the hidden layers' bias
// gradients are stage 2's to produce (the split-precision kernel leaves them to the weight-gradient kernel).
// Stage 2: the three weight-gradient GEMMs on that Ybar (split-precision or fp32 instructions), on the same stream.
static bool warp_bwd_stage1(const MlpRoute& rt, const float* params, const float* pts, const float* acts, const float* out_grad,
                            const int32_t* count, int capacity, float out_range, float* scratch, float* params_grad, float* pts_grad,
                            hipStream_t st) {
  const bool sb = rt.runs_split(2);
  if (sb) pp_launch_warp_fused_bwd_s(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, st, rt.wgs,
                                     mlp_pack_for(rt, params, 0), ordered_part(rt, 2), warp_lean_for(rt, acts, scratch) != nullptr);
  else pp_launch_warp_fused_bwd(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, st, rt.wgs);
  return sb;
}
// the split-precision weight-gradient chain of rgbnet (part: its region of an ordered workspace, or nullptr)
static void rgb_wgrad_chain_s(const float* feat, const float* acts, const float* scratch, const int32_t* count, int capacity,
                              float* pg, bool sb, hipStream_t st, int wgs, float* part) {
  const size_t FLS = (size_t)capacity * 128;
  float *b2 = sb ? pg + RGF_B2 : nullptr, *b1 = sb ? pg + RGF_B1 : nullptr, *b0 = sb ? pg + RGF_B0 : nullptr;
  pp_launch_wgrad_chain_s(scratch, acts + FLS, pg + RGF_W2, scratch + FLS, acts, pg + RGF_W1, scratch + 2 * FLS, feat, pg + RGF_W0,
                          64, count, 1, capacity, st, wgs, b2, b1, b0, part, nullptr);
}

// Join scope of the weight gradients (pp_wgrad_join_begin).  Inside it pp_rgbnet_bwd leaves its weight-gradient chain
// as a record in the context - nothing but the optimiser reads those gradients - and the next warp chain on that context carries
// the three products in its own launch (k_wgrad_join_s).  Whatever cannot be joined is launched exactly as outside the scope.
// the pending chain of `c` in a launch of its own, as pp_rgbnet_bwd would have made it
static void wgrad_join_flush(PPContext* c, int wgs) {
  if (!c->join_pending) return;
  c->join_pending = false;
  rgb_wgrad_chain_s(c->join.feat, c->join.acts, c->join.scratch, c->join.count, c->join.capacity, c->join.params_grad, true,
                    c->join.stream, wgs, nullptr);
}
// pp_rgbnet_bwd behind its data-gradient kernel: is the chain left to the next warp chain?  Only the split-precision chain with
// float atomics whose bias sums are stage 2's (sb) can ride; a record nobody took is launched first
static bool wgrad_join_defer(void* ctx, const MlpRoute& rt, bool sb, const float* feat, const float* acts, const float* scratch,
                             const int32_t* count, int capacity, float* params_grad, hipStream_t st) {
  PPContext* c = static_cast<PPContext*>(ctx);
  if (!c || !c->join_open || !sb || !rt.runs_split(16) || c->ord) return false;
  wgrad_join_flush(c, rt.wgs);
  c->join.feat = feat; c->join.acts = acts; c->join.scratch = scratch;
  c->join.count = count; c->join.capacity = capacity; c->join.params_grad = params_grad; c->join.stream = st;
  c->join_pending = true;
  return true;
}
// a warp chain about to be launched: does the pending record ride in it?  Only in the lean form of the split-precision chain with
// float atomics and bias sums (sb), for the same `count` and stream; otherwise the pending chain is launched on its own, now
static bool wgrad_join_rides(void* ctx, const MlpRoute& rt, const float* acts, const float* scratch, const int32_t* count, bool sb,
                             hipStream_t st) {
  PPContext* c = static_cast<PPContext*>(ctx);
  if (!c || !c->join_pending) return false;
  if (sb && !c->ord && rt.runs_split(16) && warp_lean_for(rt, acts, scratch) && c->join.count == count && c->join.stream == st)
    return true;
  wgrad_join_flush(c, rt.wgs);
  return false;
}

extern "C" int pp_wgrad_join_end(void* ctx, int32_t launch_pending) {
  PP_REQUIRE(ctx, "null context");
  PPContext* c = static_cast<PPContext*>(ctx);
  c->join_open = false;
  if (launch_pending) {
    wgrad_join_flush(c, MlpRoute(ctx).wgs);
    PP_CHECK_LAUNCH();
  }
  c->join_pending = false;
  return PP_OK;
}

extern "C" int pp_wgrad_join_begin(void* ctx) {
  PP_REQUIRE(ctx, "null context (the scope is recorded in a context: create one)");
  const int status = pp_wgrad_join_end(ctx, 1);
  if (status != PP_OK) return status;
  static_cast<PPContext*>(ctx)->join_open = true;
  return PP_OK;
}

// join (wgrad_join_rides said so): the pending rgbnet chain of context `jc` rides in this launch
static void warp_bwd_stage2(const MlpRoute& rt, const float* acts, const float* scratch, const int32_t* count, int capacity,
                            float* params_grad, bool sb, hipStream_t st, PPContext* jc = nullptr) {
  const int rcap = capacity * 4;
  const size_t LS = (size_t)rcap * 128;
  float *pg = params_grad, *b3 = sb ? pg + WPF_B3 : nullptr, *b2 = sb ? pg + WPF_B2 : nullptr, *b1 = sb ? pg + WPF_B1 : nullptr;
  // inside a lean scope slot 0 of `scratch` holds the output gradients and X0 only its primal rows: the kernel rebuilds the rest
  const float* lp = warp_lean_for(rt, acts, scratch);
  const WgradLean lean{acts + 3 * LS, lp ? lp + WPF_W4 : nullptr, lp ? lp + WPF_W0 : nullptr};
  if (jc) {
    jc->join_pending = false;
    const size_t FLS = (size_t)jc->join.capacity * 128;
    const float *ra = jc->join.acts, *rs = jc->join.scratch;
    float* rg = jc->join.params_grad;
    const WgradOperands warp3[3] = {{scratch, acts + 2 * LS, pg + WPF_W3, b3}, {scratch + LS, acts + LS, pg + WPF_W2, b2},
                                    {scratch + 2 * LS, acts, pg + WPF_W1, b1}};
    const WgradOperands rgb3[3] = {{rs, ra + FLS, rg + RGF_W2, rg + RGF_B2}, {rs + FLS, ra, rg + RGF_W1, rg + RGF_B1},
                                   {rs + 2 * FLS, jc->join.feat, rg + RGF_W0, rg + RGF_B0}};
    pp_launch_wgrad_join_s(warp3, rgb3, count, rcap, jc->join.capacity, st, rt.wgs, lean);
    return;
  }
  if (rt.runs_split(16))
    pp_launch_wgrad_chain_s(scratch, acts + 2 * LS, pg + WPF_W3, scratch + LS, acts + LS, pg + WPF_W2, scratch + 2 * LS, acts, pg + WPF_W1,
                            128, count, 4, rcap, st, rt.wgs, b3, b2, b1, ordered_part(rt, 0), lp ? &lean : nullptr);
  else
    pp_launch_wgrad_chain(scratch, acts + 2 * LS, pg + WPF_W3, scratch + LS, acts + LS, pg + WPF_W2, scratch + 2 * LS, acts, pg + WPF_W1,
                          128, count, 4, rcap, st, rt.wgs, b3, b2, b1);
}
static bool rgb_bwd_stage1(const MlpRoute& rt, const float* params, const float* acts, const float* rgb, const float* rgb_grad,
                           const int32_t* count, int capacity, float* scratch, float* params_grad, float* feat_grad, float* logit_grad,
                           int lg_ld, hipStream_t st) {
  const bool sb = rt.runs_split(8);
  if (sb) pp_launch_rgb_fused_bwd_s(params, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, logit_grad, lg_ld,
                                    st, rt.wgs, mlp_pack_for(rt, params, 1), ordered_part(rt, 3));
  else pp_launch_rgb_fused_bwd(params, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, logit_grad, lg_ld, st, rt.wgs);
  return sb;
}
static void rgb_bwd_stage2(const MlpRoute& rt, const float* feat, const float* acts, const float* scratch, const int32_t* count,
                           int capacity, float* params_grad, bool sb, hipStream_t st) {
  const size_t FLS = (size_t)capacity * 128;
  float *pg = params_grad, *b2 = sb ? pg + RGF_B2 : nullptr, *b1 = sb ? pg + RGF_B1 : nullptr, *b0 = sb ? pg + RGF_B0 : nullptr;
  if (rt.runs_split(16))
    rgb_wgrad_chain_s(feat, acts, scratch, count, capacity, pg, sb, st, rt.wgs, ordered_part(rt, 1));
  else
    pp_launch_wgrad_chain(scratch, acts + FLS, pg + RGF_W2, scratch + FLS, acts, pg + RGF_W1, scratch + 2 * FLS, feat, pg + RGF_W0,
                          64, count, 1, capacity, st, rt.wgs, b2, b1, b0);
}

// may_defer (pp_rgbnet_bwd): inside a join scope the weight-gradient chain may be left to the next warp chain (wgrad_join_defer)
static int pp_mlp_bwd_impl(const float* params, const float* feat, int32_t in_ld, int32_t n_gemm, const float* acts, const float* out,
                           const float* out_grad, const int32_t* count, int32_t capacity, float* scratch, float* params_grad,
                           float* feat_grad, float* logit_add_grad, int32_t logit_add_ld, void* ctx, void* stream, bool may_defer) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && feat && acts && out && out_grad && count && scratch && params_grad, "null pointer");
  PP_REQUIRE(capacity > 0 && in_ld % 32 == 0 && in_ld <= 128 && n_gemm >= 1 && n_gemm <= 8, "bad sizes");
  PP_REQUIRE_ORDERED(rt, capacity, 8 | 16, in_ld == 64 && n_gemm == 3 && feat_grad != nullptr);
  hipStream_t st = pp_stream(stream);
  if (in_ld == 64 && n_gemm == 3 && feat_grad && rt.fused) {
    const bool sb = rgb_bwd_stage1(rt, params, acts, out, out_grad, count, capacity, scratch, params_grad, feat_grad, logit_add_grad,
                                   logit_add_ld, st);
    if (!(may_defer && wgrad_join_defer(ctx, rt, sb, feat, acts, scratch, count, capacity, params_grad, st)))
      rgb_bwd_stage2(rt, feat, acts, scratch, count, capacity, params_grad, sb, st);
  } else
    pp_launch_mlp_layered_bwd(params, feat, in_ld, n_gemm, acts, out, out_grad, count, capacity, scratch, params_grad, feat_grad,
                              logit_add_grad, logit_add_ld, st);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_mlp_bwd(const float* params, const float* feat, int32_t in_ld, int32_t n_gemm, const float* acts,
                          const float* out, const float* out_grad, const int32_t* count, int32_t capacity,
                          float* scratch, float* params_grad, float* feat_grad, float* logit_add_grad,
                          int32_t logit_add_ld, void* ctx, void* stream) {
  return pp_mlp_bwd_impl(params, feat, in_ld, n_gemm, acts, out, out_grad, count, capacity, scratch, params_grad, feat_grad,
                         logit_add_grad, logit_add_ld, ctx, stream, false);
}

// rgbnet of the Voxurf configuration = generic MLP with a 64-wide (57 used) input and three 128-wide layers.
extern "C" int pp_rgbnet_fwd(const float* params, const float* feat, const int32_t* count, int32_t capacity,
                             float* acts, float* rgb, void* ctx, void* stream) {
  return pp_mlp_fwd(params, feat, 64, 3, count, capacity, nullptr, 0, acts, rgb, ctx, stream);
}

extern "C" int pp_rgbnet_bwd(const float* params, const float* feat, const float* acts, const float* rgb,
                             const float* rgb_grad, const int32_t* count, int32_t capacity, float* scratch,
                             float* params_grad, float* feat_grad, void* ctx, void* stream) {
  PP_REQUIRE(feat_grad, "null pointer");
  return pp_mlp_bwd_impl(params, feat, 64, 3, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, nullptr, 0,
                         ctx, stream, true);
}

extern "C" int pp_warp_fwd(const float* params, const float* pts, const int32_t* count, int32_t capacity,
                           float out_range, float* acts, float* out, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && pts && count && out, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE(acts || rt.runs_split(1),
             "acts may be NULL (forward only) only with the split-precision forward kernel (option mlp_split bit 1)");
  hipStream_t st = pp_stream(stream);
  if (!rt.fused) pp_launch_warp_layered_fwd(params, pts, count, capacity, out_range, acts, out, st);
  else if (rt.runs_split(1))
    pp_launch_warp_fused_fwd_s(params, pts, count, capacity, out_range, acts, out, st, rt.wgs, mlp_pack_for(rt, params, 0),
                               acts && warp_lean_for(rt, acts, nullptr) != nullptr);
  else pp_launch_warp_fused_fwd(params, pts, count, capacity, out_range, acts, out, st, rt.wgs);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_warp_bwd(const float* params, const float* pts, const float* acts, const float* out_grad,
                           const int32_t* count, int32_t capacity, float out_range, float* scratch,
                           float* params_grad, float* pts_grad, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && pts && acts && out_grad && count && scratch && params_grad && pts_grad, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  PP_REQUIRE_ORDERED(rt, capacity, 2 | 16);
  hipStream_t st = pp_stream(stream);
  // a pending rgbnet chain of this context (pp_wgrad_join_begin) rides in stage 2, or is launched on its own first
  const bool ride = wgrad_join_rides(ctx, rt, acts, scratch, count, rt.runs_split(2), st);
  if (rt.fused) {
    // one fused data-gradient kernel (+ thin layers), then the three weight-gradient GEMMs on the Ybar it left behind
    const bool sb = warp_bwd_stage1(rt, params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, st);
    warp_bwd_stage2(rt, acts, scratch, count, capacity, params_grad, sb, st, ride ? static_cast<PPContext*>(ctx) : nullptr);
  } else
    pp_launch_warp_layered_bwd(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, st);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Two-stage forms of the layer-fused backward chains: the data-gradient kernel (which also produces the thin layers' and
// all bias gradients and leaves Ybar of the hidden layers in `scratch`) and the weight-gradient kernel are separate entry
// points, so that a caller can time them or place other work between them on the stream.
// pp_warp_bwd / pp_rgbnet_bwd are exactly stage 1 followed by stage 2.
// ------------------------------------------------------------------------------------------------------------------
extern "C" int pp_warp_bwd_data(const float* params, const float* pts, const float* acts, const float* out_grad,
                                const int32_t* count, int32_t capacity, float out_range, float* scratch,
                                float* params_grad, float* pts_grad, int32_t* stage2_host, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && pts && acts && out_grad && count && scratch && params_grad && pts_grad && stage2_host, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  if (!rt.fused) { pp_set_error("pp_warp_bwd_data: option mlp_fused = 0 has no two-stage form"); return PP_ERR_UNSUPPORTED; }
  PP_REQUIRE_ORDERED(rt, capacity, 2);
  // 1: the hidden layers' bias gradients are stage 2's to produce
  *stage2_host = warp_bwd_stage1(rt, params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad,
                                 pp_stream(stream)) ? 1 : 0;
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_warp_bwd_weights(const float* acts, const float* scratch, const int32_t* count, int32_t capacity,
                                   float* params_grad, int32_t stage2, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(acts && scratch && count && params_grad, "null pointer");
  PP_REQUIRE(capacity > 0 && (stage2 == 0 || stage2 == 1), "capacity<=0 or stage2 is not what pp_warp_bwd_data returned");
  if (!rt.fused) { pp_set_error("pp_warp_bwd_weights: option mlp_fused = 0 has no two-stage form"); return PP_ERR_UNSUPPORTED; }
  PP_REQUIRE_ORDERED(rt, capacity, 16);
  // who owns b1..b3 was decided by stage 1 and is handed over explicitly (never re-read from the options)
  // (a pending rgbnet chain of this context rides, or is launched on its own first: pp_wgrad_join_begin)
  const bool ride = wgrad_join_rides(ctx, rt, acts, scratch, count, stage2 != 0, pp_stream(stream));
  warp_bwd_stage2(rt, acts, scratch, count, capacity, params_grad, stage2 != 0, pp_stream(stream),
                  ride ? static_cast<PPContext*>(ctx) : nullptr);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_rgbnet_bwd_data(const float* params, const float* acts, const float* rgb, const float* rgb_grad,
                                  const int32_t* count, int32_t capacity, float* scratch, float* params_grad,
                                  float* feat_grad, int32_t* stage2_host, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(params && acts && rgb && rgb_grad && count && scratch && params_grad && feat_grad && stage2_host, "null pointer");
  PP_REQUIRE(capacity > 0, "capacity<=0");
  if (!rt.fused) { pp_set_error("pp_rgbnet_bwd_data: option mlp_fused = 0 has no two-stage form"); return PP_ERR_UNSUPPORTED; }
  PP_REQUIRE_ORDERED(rt, capacity, 8);
  *stage2_host = rgb_bwd_stage1(rt, params, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, nullptr, 0,
                                pp_stream(stream)) ? 1 : 0;
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_rgbnet_bwd_weights(const float* feat, const float* acts, const float* scratch, const int32_t* count,
                                     int32_t capacity, float* params_grad, int32_t stage2, void* ctx, void* stream) {
  const MlpRoute rt(ctx);
  PP_REQUIRE(feat && acts && scratch && count && params_grad, "null pointer");
  PP_REQUIRE(capacity > 0 && (stage2 == 0 || stage2 == 1), "capacity<=0 or stage2 is not what pp_rgbnet_bwd_data returned");
  if (!rt.fused) { pp_set_error("pp_rgbnet_bwd_weights: option mlp_fused = 0 has no two-stage form"); return PP_ERR_UNSUPPORTED; }
  PP_REQUIRE_ORDERED(rt, capacity, 16);
  rgb_bwd_stage2(rt, feat, acts, scratch, count, capacity, params_grad, stage2 != 0, pp_stream(stream));   // see pp_warp_bwd_weights
  PP_CHECK_LAUNCH();
  return PP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Workspace queries: floats the caller must provide for `acts` (kept from forward to backward) and `scratch` (backward
// only) of the MLP entry points at a given sample capacity.
// ------------------------------------------------------------------------------------------------------------------
extern "C" int pp_rgbnet_workspace(int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats) {
  PP_REQUIRE(acts_floats && scratch_floats && capacity > 0, "bad arguments");
  *acts_floats = (int64_t)3 * capacity * 128;
  *scratch_floats = (int64_t)3 * capacity * 128 + 49152;          // Ybar of the three hidden layers (+ transposed weights, layered path)
  return PP_OK;
}

extern "C" int pp_warp_workspace(int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats) {
  PP_REQUIRE(acts_floats && scratch_floats && capacity > 0, "bad arguments");
  *acts_floats = (int64_t)4 * capacity * 4 * 128;                 // four hidden activations of the 4-row form
  *scratch_floats = (int64_t)3 * capacity * 4 * 128 + 49152;
  return PP_OK;
}

extern "C" int pp_mlp_workspace(int32_t in_ld, int32_t n_gemm, int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats) {
  PP_REQUIRE(acts_floats && scratch_floats && capacity > 0 && in_ld % 32 == 0 && in_ld <= 128 && n_gemm >= 1 && n_gemm <= 8,
             "bad arguments");
  *acts_floats = (int64_t)n_gemm * capacity * 128;
  *scratch_floats = (int64_t)(n_gemm > 3 ? n_gemm : 3) * capacity * 128 + 49152;
  return PP_OK;
}
