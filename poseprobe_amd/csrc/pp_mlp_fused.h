// Internal interface between pp_mlp.hip (C-ABI entry points, routing) and the kernels of the object-branch MLPs: pp_mlp_fused.hip,
// pp_mlp_split.hip (layer-fused), pp_mlp_layered.hip.  A launcher reads no option: what the entry point resolved comes in as arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// parameter block of the warp net: W0[128x3] b0 | W1..W3[128x128] b | W4[4x128] b4   (poseprobe_amd/engine.py FlatParams)
#define WPF_W0 0
#define WPF_B0 (128 * 3)
#define WPF_W1 (WPF_B0 + 128)
#define WPF_B1 (WPF_W1 + 128 * 128)
#define WPF_W2 (WPF_B1 + 128)
#define WPF_B2 (WPF_W2 + 128 * 128)
#define WPF_W3 (WPF_B2 + 128)
#define WPF_B3 (WPF_W3 + 128 * 128)
#define WPF_W4 (WPF_B3 + 128)
#define WPF_B4 (WPF_W4 + 4 * 128)

// wgs (every launcher of a layer-fused kernel): the call's persistent work-group count (MlpRoute, pp_mlp.hip); a kernel whose
// work has fewer units than that gets one work-group per unit
static inline int pp_fused_grid(int units, int wgs) { return units < wgs ? units : wgs; }

int pp_launch_warp_fused_fwd(const float* params, const float* pts, const int32_t* count, int capacity, float out_range,
                             float* acts, float* out, hipStream_t st, int wgs);
int pp_launch_warp_fused_bwd(const float* params, const float* pts, const float* acts, const float* out_grad,
                             const int32_t* count, int capacity, float out_range, float* ybar, float* params_grad,
                             float* pts_grad, hipStream_t st, int wgs);
// operands of one layer of the weight-gradient chain (split-precision kernel, pp_mlp_split.hip)
struct WgradOperands {
  const float* Y;      // [R][128]  gradient w.r.t. the layer's pre-activation (already gated)
  const float* X;      // [R][KX]   input activations of the layer
  float* Wbar;         // [128][KX]
  float* bbar;         // [128] or nullptr: += column sums of Y (every row, or the primal rows of the 4-row form)
};
// what the lean form of the warp net's chain (pp_warp_lean_begin) needs beside the operands: layer A's Y then holds the 16 output
// gradients per sample and Ybar3 is rebuilt from them, W4 and the gate; layer C's tangent rows of X0 are rebuilt from W0
struct WgradLean {
  const float* gate3;  // X3 [R][128]: its primal rows gate the rebuilt Ybar3
  const float* w4;     // W4 [4][128]
  const float* w0;     // W0 [128][3]
};
int pp_launch_wgrad_chain_s(const float* YA, const float* XA, float* WA, const float* YB, const float* XB, float* WB,
                            const float* YC, const float* XC, float* WC, int kxc, const int32_t* count, int rmul, int rcap,
                            hipStream_t st, int wgs, float* bA, float* bB, float* bC, float* part, const WgradLean* lean);
// the weight gradients of both nets in one launch (k_wgrad_join_s; pp_wgrad_join_begin): warp3 = the warp net's three layers in
// lean form (4 count rows, capacity rcap_w), rgb3 = rgbnet's (count rows, capacity rcap_r; rgb3[2] is the 64-wide input layer),
// all with bias sums; float atomics only
int pp_launch_wgrad_join_s(const WgradOperands* warp3, const WgradOperands* rgb3, const int32_t* count, int rcap_w, int rcap_r,
                           hipStream_t st, int wgs_cu, const WgradLean& lean);
// split-precision variants (pp_mlp_split.hip, option "mlp_split"): same contracts.  pack: the weight pack written by
// pp_launch_mlp_pack FOR THESE params (pp_mlp_pack.h), or nullptr = the kernel derives the same quantities in its prologue.
// part (backward kernels, weight-gradient chain): this launch's region of the ordered-flush workspace (pp_ordered.h) - the
// parameter gradients are then added up in a fixed order by a reduction launched behind the kernel; nullptr = float atomics
// lean (warp net, pp_warp_lean_begin): the forward kernel leaves the tangent rows of X0 unwritten, the backward kernel writes the
// scaled output gradients to the start of `ybar` instead of Ybar3
int pp_launch_warp_fused_fwd_s(const float* params, const float* pts, const int32_t* count, int capacity, float out_range,
                               float* acts, float* out, hipStream_t st, int wgs, const float* pack, bool lean);
int pp_launch_warp_fused_bwd_s(const float* params, const float* pts, const float* acts, const float* out_grad,
                               const int32_t* count, int capacity, float out_range, float* ybar, float* params_grad,
                               float* pts_grad, hipStream_t st, int wgs, const float* pack, float* part, bool lean);
int pp_launch_mlp_pack(const float* warp_params, const float* rgbnet_params, float* pack, hipStream_t st);
// the step's scalars as a kernel argument of k_step_begin (pp_step_begin): n <= PP_STEP_SCALARS_MAX floats
#define PP_STEP_SCALARS_MAX 32
struct PPStepScalars { float v[PP_STEP_SCALARS_MAX]; int n; };
// pose forward + step scalars + zero block in work-group 0, the PK_TASKS tasks of the weight pack beside it (pack == nullptr: none)
int pp_launch_step_begin(const float* se3, const float* w2c_init, const int32_t* refine_mask, int n_views, float* w2c, float* c2w,
                         float* jac, const PPStepScalars& sv, float* step_dev, float* zero_block, int n_zero,
                         const float* warp_params, const float* rgbnet_params, float* pack, hipStream_t st);
// weight gradients of three layers (Y_l^T X_l accumulated into W_l) in one persistent kernel; kxc = width of X of layer C;
// bA / bB / bC: also accumulate the bias gradients = column sums of Y over the primal rows (kxc == 128: the warp net's 4-row
// form, every fourth row) or over all rows (kxc == 64: rgbnet)
int pp_launch_wgrad_chain(const float* YA, const float* XA, float* WA, const float* YB, const float* XB, float* WB,
                          const float* YC, const float* XC, float* WC, int kxc, const int32_t* count, int rmul, int rcap,
                          hipStream_t st, int wgs, float* bA, float* bB, float* bC);

// parameter block of rgbnet (64-wide padded input): W0[128x64] b0 | W1[128x128] b1 | W2[128x128] b2 | W3[3x128] b3
#define RGF_W0 0
#define RGF_B0 (128 * 64)
#define RGF_W1 (RGF_B0 + 128)
#define RGF_B1 (RGF_W1 + 128 * 128)
#define RGF_W2 (RGF_B1 + 128)
#define RGF_B2 (RGF_W2 + 128 * 128)
#define RGF_W3 (RGF_B2 + 128)
#define RGF_B3 (RGF_W3 + 3 * 128)

int pp_launch_rgb_fused_fwd(const float* params, const float* feat, const int32_t* count, int capacity,
                            const float* logit_add, int add_ld, float* acts, float* rgb, hipStream_t st, int wgs);
int pp_launch_rgb_fused_fwd_s(const float* params, const float* feat, const int32_t* count, int capacity,
                              const float* logit_add, int add_ld, float* acts, float* rgb, hipStream_t st, int wgs, const float* pack);
int pp_launch_rgb_fused_bwd_s(const float* params, const float* acts, const float* rgb, const float* rgb_grad,
                              const int32_t* count, int capacity, float* ybar, float* params_grad, float* feat_grad,
                              float* logit_grad, int lg_ld, hipStream_t st, int wgs, const float* pack, float* part);
int pp_launch_rgb_fused_bwd(const float* params, const float* acts, const float* rgb, const float* rgb_grad,
                            const int32_t* count, int capacity, float* ybar, float* params_grad, float* feat_grad,
                            float* logit_grad, int lg_ld, hipStream_t st, int wgs);

// layer-by-layer launch sequences (pp_mlp_layered.hip): the generic ReLU MLP in_ld -> 128 x n_gemm -> 3 and the warp net in 4-row
// form; same buffers and contracts as the entry points of pp_mlp.hip that forward to them
void pp_launch_mlp_layered_fwd(const float* params, const float* feat, int in_ld, int n_gemm, const int32_t* count, int capacity,
                               const float* logit_add, int logit_add_ld, float* acts, float* out, hipStream_t st);
void pp_launch_mlp_layered_bwd(const float* params, const float* feat, int in_ld, int n_gemm, const float* acts, const float* out,
                               const float* out_grad, const int32_t* count, int capacity, float* scratch, float* params_grad,
                               float* feat_grad, float* logit_add_grad, int logit_add_ld, hipStream_t st);
void pp_launch_warp_layered_fwd(const float* params, const float* pts, const int32_t* count, int capacity, float out_range,
                                float* acts, float* out, hipStream_t st);
void pp_launch_warp_layered_bwd(const float* params, const float* pts, const float* acts, const float* out_grad, const int32_t* count,
                                int capacity, float out_range, float* scratch, float* params_grad, float* pts_grad, hipStream_t st);
