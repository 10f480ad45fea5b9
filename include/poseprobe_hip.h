/* poseprobe_hip.h - C ABI of libposeprobe_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for PoseProbe's object-branch hot path.  It replaces the reference's pybind11
 * torch extension `render_utils_cuda` (lib/cuda/render_utils.cpp:170-184) and the eager-PyTorch op
 * chains of lib/voxurf_coarse.py / lib/dvgo_ori.py / lib/camera.py / lib/losses.py / lib/utils.py
 * listed per entry point below (file:line relative to the reference tree).
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch / ATen types;
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the CALLER owns every buffer
 *     (inputs, outputs, workspace) - the library never allocates and never synchronises;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are re-entrant;
 *   - sample counts that are data dependent (M) live in device memory (`count`, one int32) so that a
 *     whole train step can be enqueued / graph-captured without a host round trip; kernels are
 *     launched for the capacity and retire surplus work-groups immediately;
 *   - fp32 values, int32 indices (the Python shim converts to int64 where the reference returns it);
 *   - return value: 0 on success, negative pp_status otherwise; pp_last_error() gives the text of
 *     the last failure on the calling thread;
 *   - arguments are passed one by one rather than through per-op `pp_<op>_args` structs (SURVEY 8b sketched those): the binding
 *     derives its prototypes from this header and so checks count and type of every argument; scratch sizes come from the
 *     pp_*_workspace queries, option values from the caller-owned pp_context handed to the call - the library holds no
 *     process-wide mutable state (ABI 3; ABI 1 / 2 had pp_set_option).
 */
#ifndef POSEPROBE_HIP_H
#define POSEPROBE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  PP_OK = 0,
  PP_ERR_INVALID_ARG = -1,
  PP_ERR_LAUNCH = -2,
  PP_ERR_UNSUPPORTED = -3
} pp_status;

const char* pp_last_error(void);
/* ABI history.  1: round 1.  2: pp_loss_rays / pp_loss_samples / pp_geometry_bwd_priors gained `const float* batch_norm`
 * in front of `stream` (the library kept answering 1 for it by mistake).  3: options moved from process-wide
 * pp_set_option / pp_get_option into the caller-owned pp_context, which every option-dependent entry point now takes in front
 * of `stream` (pp_rgbnet_fwd, pp_warp_fwd, pp_mlp_fwd, the four two-stage backward entry points - which also hand the bias
 * ownership from stage 1 to stage 2 explicitly -, pp_nerf_fwd / pp_nerf_bwd, pp_grid_tv_adam_step{,_sparse});
 * pp_scene gained `sdf_index_exact`; new: pp_sdf_crossing_dense_bwd, pp_context_set_option / pp_context_get_option.  4 (this header): the
 * auxiliary-stream placement of the weight-gradient kernels is gone with its join entry point and its two options.
 * Entry points added without a version change (no existing signature moved): the pp_reproj_* group, the pp_featproj_* group, the pp_mc_* group, the pp_pnp_* group,
 * the pp_dtu_* group, the pp_ssim_* group, pp_step_begin, pp_march_loss_bwd / pp_march_loss_workspace, pp_geometry_plain_fwd /
 * pp_geometry_plain_bwd, pp_keep_compact / pp_keep_scatter_bwd, pp_vertex_feat, the pp_cc_* group, the pp_msdf_* group.
 * A binding MUST compare pp_abi_version() with the PP_ABI_VERSION it was built against before calling anything else
 * (poseprobe_amd/_lib.py does): the signatures changed, so a stale caller would pass a stream where a pointer is read. */
#define PP_ABI_VERSION 4
int pp_abi_version(void);

/* Static description of the voxel scene; mirrors the attributes Voxurf derives in __init__ /
 * _set_grid_resolution (lib/voxurf_coarse.py:67-68, :319-323) and the render_kwargs
 * (lib/recon_scene.py:208-217). */
typedef struct {
  float xyz_min[3];
  float xyz_max[3];
  int32_t size[3];      /* world_size X,Y,Z */
  float voxel_size;     /* fp32 value of Voxurf.voxel_size */
  float stepsize;       /* in voxels */
  float near_clip;
  float far_clip;
  float bg;
  int32_t n_samples;    /* S = int(|world_size+1| / stepsize) + 1  (voxurf_coarse.py:700) */
  float out_range;      /* DeformedImplicitField.output_range (deform_net.py:17) */
  int32_t k0_dim;       /* 12 */
  int32_t pos_pe;       /* 5 */
  int32_t view_pe;      /* 1 */
  int32_t sdf_index_exact; /* 0: the custom SDF sampler forms the flat voxel index in fp32 like the reference (differs above 2^24
                            * voxels only, lib/voxurf_coarse.py:632-647); 1: the mathematically intended index */
} pp_scene;

/* ---------------------------------------------------------------- pose: lib/camera.py:76-99,127-188;
 * lib/recon_scene.py:62-74 (get_current_pose_pnp) + camera.pose.invert (recon_scene.py:444).
 * se3[V,6], w2c_init[V,3,4] -> w2c[V,3,4], c2w[V,3,4]; jac[V,12,6] = d c2w / d se3 (forward mode),
 * consumed by pp_pose_bwd: se3_grad[V,6] = jac^T c2w_grad.  refine_mask[V] (0 = view is not refined). */
int pp_pose_fwd(const float* se3, const float* w2c_init, const int32_t* refine_mask, int32_t n_views,
                float* w2c, float* c2w, float* jac, void* stream);
int pp_pose_bwd(const float* jac, const float* c2w_grad, int32_t n_views, float* se3_grad, void* stream);

/* ---------------------------------------------------------------- rays: lib/voxurf_coarse.py:1339-1368,
 * :1402-1407, :1518-1549 + the randperm selection (recon_scene.py:598-600), index-first: only the selected
 * pixels are generated.  ray_idx[N] indexes the flattened [V,H,W] pixel list.  normalize=1: Voxurf
 * variant (rays_d = viewdirs), 0: DVGO variant (dvgo_ori.py:562-563).  images[V,H,W,3], masks[V,H,W].
 * Also performs the slab test of sample_ray_ori (voxurf_coarse.py:702-708): t_min,t_max[N]. */
int pp_raygen_select_fwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                         const float* intr /*[V,4] fx,fy,cx,cy*/, int32_t n_views, int32_t H, int32_t W,
                         int32_t inverse_y, int32_t normalize, const float* images, const float* masks,
                         float* rays_o, float* rays_d, float* viewdirs, float* target, float* mask_px,
                         void* stream);
/* Backward of the above plus of the dense sampler's ray-level terms: consumes per-sample gradients
 * (pts_grad[M,3], step[M], viewdir_grad_s[M,3]) segmented by ray_start[N+1], optional direct grads
 * on rays (may be NULL); produces per-ray grads rays_o/rays_d/viewdirs_grad_out[N,3] (any may be NULL) and,
 * when c2w_grad != NULL (Voxurf ray variant), c2w_grad[V,3,4] (zeroed by the callee). */
int pp_raygen_select_bwd(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                         const float* intr, int32_t n_views, int32_t H, int32_t W, int32_t inverse_y,
                         const float* rays_o, const float* rays_d, const float* t_min,
                         const int32_t* ray_start, const float* pts_grad, const float* step,
                         const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                         const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out,
                         float* rays_d_grad_out, float* viewdirs_grad_out, float* c2w_grad, void* stream);

/* ---------------------------------------------------------------- dense sampler + compaction:
 * Voxurf.sample_ray_ori (voxurf_coarse.py:697-719) followed by the boolean compaction (:936-945).
 * jitter[N] may be NULL (eval).  Outputs: t_min,t_max[N], ray_start[N+1] (exclusive prefix of the
 * per-ray in-bbox counts; ray_start[N] = M, also written to count[0]), pts[M,3], ray_id[M],
 * step_k[M] (sample index within the ray), step[M] (= stepsize*voxel_size*(k+jitter)),
 * mask_keep[N*S] (uint8, 1 = in bbox; may be NULL).  capacity = allocated rows of the per-sample outputs: when the in-bbox
 * total exceeds it, count[0] = ray_start[N] = capacity and every ray_start entry is clamped to it (rays past the capacity
 * become empty, the ray that straddles it is cut), so no consumer of ray_start ever indexes past the allocation;
 * count[0] == capacity is the caller's truncation signal.  The same holds for pp_sample_var. */
int pp_sample_dense(const pp_scene* sc, const float* rays_o, const float* rays_d, const float* jitter,
                    int32_t n_rays, int32_t capacity, float* t_min, float* t_max, int32_t* ray_start,
                    int32_t* count, float* pts, int32_t* ray_id, int32_t* step_k, float* step,
                    uint8_t* mask_keep, void* stream);

/* Variable-length sampler of the reference's CUDA extension: sample_pts_on_rays
 * (lib/cuda/render_utils_kernel.cu:12-242) as used by Voxurf.sample_ray_cuda (voxurf_coarse.py:661-695,
 * far forced to 1e9, points recomputed as rays_start + dir*step_id*stepdist, in-bbox compaction).
 * n_steps[N] are the raw per-ray counts (kernel.cu:38-55); ray_start[N+1] prefix of the kept samples. */
int pp_sample_var(const pp_scene* sc, const float* rays_o, const float* rays_d, int32_t n_rays,
                  int32_t capacity, float* t_min, float* t_max, int32_t* n_steps, int32_t* ray_start,
                  int32_t* count, float* pts, int32_t* ray_id, int32_t* step_id, void* stream);

/* ---------------------------------------------------------------- transmittance scan:
 * render_utils_cuda.alpha2weight / alpha2weight_backward (lib/cuda/render_utils_kernel.cu:577-707, bound
 * at lib/voxurf_coarse.py:1319,:1329).  ray_start[N+1] replaces the kernel's i_start/i_end bookkeeping
 * (kernel.cu:607-636).  One wavefront per ray; sequential-order products, 1e-3 early stop. */
int pp_alpha2weight_fwd(const float* alpha, const int32_t* ray_start, int32_t n_rays, float* weights,
                        float* T, float* alphainv_last, int32_t* i_end, void* stream);
int pp_alpha2weight_bwd(const float* alpha, const float* weights, const float* T, const float* alphainv_last,
                        const int32_t* ray_start, const int32_t* i_end, int32_t n_rays,
                        const float* grad_weights, const float* grad_last, float* grad_alpha, void* stream);

/* Fused scan + compositing (replaces Alphas2Weights + the segment_coo calls, voxurf_coarse.py:995,
 * :1034-1057 / inference :1179-1202): rgb_marched[N,3] (clamped), rgb_pre[N,3] (pre-clamp, for the
 * backward), cum_weights[N], depth_acc[N] = sum w*step_w (step_w[M]: train `step`, inference
 * step_id*dist), optional normal_marched[N,3] from nrm_in[M,3] (may be NULL). */
int pp_march_fwd(const float* alpha, const float* rgb, const float* step_w, const float* nrm_in,
                 const int32_t* ray_start, int32_t n_rays, float bg, float* weights, float* T,
                 float* alphainv_last, int32_t* i_end, float* rgb_marched, float* rgb_pre,
                 float* cum_weights, float* depth_acc, float* normal_marched, void* stream);
int pp_march_bwd(const float* alpha, const float* rgb, const float* step_w, const float* weights, const float* T,
                 const float* alphainv_last, const int32_t* ray_start, const int32_t* i_end, int32_t n_rays,
                 float bg, const float* rgb_pre, const float* g_rgb_marched, const float* g_cum_weights,
                 const float* g_alphainv_last, const float* g_depth_acc, const float* g_weights /*[M] or NULL*/,
                 float* grad_alpha, float* grad_rgb, void* stream);

/* ---------------------------------------------------------------- geometry: sdf mapping
 * (voxurf_coarse.py:946-949), custom trilinear lookup at deformed / undeformed points (:545-659, :967,
 * :978), spatial gradients (:968-984) and NeuS alpha (:483-519), fused.  The mapped grid is never
 * materialised: the 8 corner values are mapped in registers.
 * warp_out[M,4,4]: row 0 = (deform xyz, correction), rows 1-3 = d/dp_i of the same (already x out_range).
 * Outputs: alpha[M], gradient[M,3], sdf_final[M], sdf_deform[M], grad_deform[M,3,3]. */
int pp_geometry_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab /*[2] raw alpha,beta*/,
                    const float* pts, const float* warp_out, const float* viewdirs, const int32_t* ray_id,
                    const int32_t* count, int32_t capacity, float inv_s, float* alpha, float* gradient,
                    float* sdf_final, float* sdf_deform, float* grad_deform, void* stream);
/* Upstream grads (any may be NULL): g_alpha[M], g_gradient[M,3], g_sdf_final[M], g_sdf_deform[M],
 * g_grad_deform[M,9], g_correction[M].  Outputs: warp_out_grad[M,4,4], pts_grad[M,3] (accumulate=1: +=),
 * viewdir_grad_s[M,3] (+= if accumulate), sdf_ab_grad[2] (atomic +=; caller zeroes). */
int pp_geometry_bwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                    const float* warp_out, const float* viewdirs, const int32_t* ray_id, const int32_t* count,
                    int32_t capacity, float inv_s, const float* g_alpha, const float* g_gradient,
                    const float* g_sdf_final, const float* g_sdf_deform, const float* g_grad_deform,
                    const float* g_correction, int32_t accumulate, float* warp_out_grad, float* pts_grad,
                    float* viewdir_grad_s, float* sdf_ab_grad, void* stream);

/* pp_geometry_bwd + pp_loss_samples in one kernel: the four sample-level priors of object_losses (lib/losses.py:6-23) are
 * evaluated from the recomputed forward, their values accumulated into loss_out[2..5] (as pp_loss_samples does) and
 * their gradients folded into the backward without the g_grad_deform / g_correction / g_sdf_deform round trip through
 * HBM.  g_gradient[M,3] = upstream gradient of the normal from the colour features (may be NULL).  Bit-identical to the
 * two-call sequence (except loss_out[7], the weighted total, which only pp_loss_rays / pp_loss_samples maintain). */
int pp_geometry_bwd_priors(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                           const float* warp_out, const float* viewdirs, const int32_t* ray_id, const int32_t* count,
                           int32_t capacity, float inv_s, const float* g_alpha, const float* g_gradient, float w_eikonal,
                           float w_deform, float loss_scale, int32_t accumulate, float* warp_out_grad, float* pts_grad,
                           float* viewdir_grad_s, float* sdf_ab_grad, float* loss_out, const float* batch_norm,
                           void* stream);

/* ---------------------------------------------------------------- multi-GPU: k0 gradient exchange at sample granularity
 * (no counterpart in the reference, which has no distributed path; replaces a dense 196 MB reduce-scatter by an
 * all-gather of 64 B per sample).  pp_k0_pack_samples writes packed[capacity][16] = { feat_grad[:, :k0_dim] (12 slots),
 * pts xyz, pad } and the sample count (int32 bit pattern) into packed[0][15]; pp_k0_scatter_packed replays the trilinear
 * scatter of pp_color_feat_bwd for n_shards such buffers laid out back to back ([n_shards][capacity][16]) into
 * k0_grad_cl (atomic +=).  Pass k0_grad_cl = NULL to pp_color_feat_bwd to skip its own scatter. */
int pp_k0_pack_samples(const float* pts, const float* feat_grad, const int32_t* count, int32_t capacity, int32_t k0_dim,
                       float* packed, void* stream);
int pp_k0_scatter_packed(const pp_scene* sc, const float* packed, int32_t n_shards, int32_t capacity, float* k0_grad_cl,
                         uint8_t* touched /*optional: see pp_grid_tv_adam_step_sparse*/, void* stream);
/* The scatter half of pp_color_feat_bwd on its own (same kernel), optionally marking the voxels it reaches in a map of
 * one byte per voxel (index = (x*Y + y)*Z + z; plain stores of 1, no atomics). */
int pp_k0_scatter_samples(const pp_scene* sc, const float* pts, const int32_t* count, int32_t capacity,
                          const float* feat_grad, float* k0_grad_cl, uint8_t* touched /*optional*/, void* stream);

/* Deterministic variants of the two scatters above: the (sample, corner) contributions are sorted by voxel (stable radix sort) and
 * added per voxel in ascending (shard, sample, corner) order - bit-identical results for identical inputs, from run to run and
 * between ranks that replay the same shards (float atomics retire in hardware order).  About 6 x the time of the atomic kernels:
 * an option.  `work`: device memory of pp_k0_scatter_sorted_workspace(n_shards * capacity) bytes; grids up to 2^32 - 2 voxels. */
int pp_k0_scatter_sorted_workspace(int64_t n_samples, int64_t* bytes);
int pp_k0_scatter_samples_sorted(const pp_scene* sc, const float* pts, const int32_t* count, int32_t capacity,
                                 const float* feat_grad, float* k0_grad_cl, uint8_t* touched /*optional*/, void* work,
                                 int64_t work_bytes, void* stream);
int pp_k0_scatter_packed_sorted(const pp_scene* sc, const float* packed, int32_t n_shards, int32_t capacity, float* k0_grad_cl,
                                uint8_t* touched /*optional*/, void* work, int64_t work_bytes, void* stream);

/* ---------------------------------------------------------------- colour features: DenseGrid.forward for k0
 * (lib/grid.py:47-58, zeros padding), BARF positional encoding of xyz and view (voxurf_coarse.py:721-732,
 * :1009-1025), normal (:1028-1030) -> feat[M,64] (57 used, zero padded).  k0 is stored channels-last
 * [X,Y,Z,C].  pe_w[pos_pe + view_pe] are the c2f weights for this step. */
int pp_color_feat_fwd(const pp_scene* sc, const float* k0_cl, const float* pts, const float* viewdirs,
                      const int32_t* ray_id, const float* gradient, const float* pe_w, const int32_t* count,
                      int32_t capacity, float* feat, void* stream);
/* feat_grad[M,64] -> k0_grad_cl (atomic +=), pts_grad[M,3] (=), gradient_grad[M,3] (=),
 * viewdir_grad_s[M,3] (=). */
int pp_color_feat_bwd(const pp_scene* sc, const float* k0_cl, const float* pts, const float* viewdirs,
                      const int32_t* ray_id, const float* gradient, const float* pe_w, const int32_t* count,
                      int32_t capacity, const float* feat_grad, float* k0_grad_cl, float* pts_grad,
                      float* gradient_grad, float* viewdir_grad_s, void* stream);

/* Caller-owned context = the option values of the calls it is handed to.  NULL everywhere = the compiled-in defaults (the
 * measured best on MI355X).  Options are plain integers
 * set by name; a call reads them from ITS context for the duration of the call only, so contexts with different arithmetic
 * coexist in one process and on concurrent threads (a context itself must not be modified while a call uses it).
 * Names (meaning and ranges: csrc/pp_common.h, csrc/pp_error.hip):
 *   arithmetic   mlp_split (bit mask: object-branch MLP kernels as 3 fp16 products per fp32 product; 0 = fp32 MFMA instructions),
 *                nerf_split (scene branch likewise), mlp_fused,
 *                nerf_chain (scene branch: 3 = the fused forward and backward chains, 0 = one GEMM per layer; nothing in between)
 *   scheduling   mlp_wgs, grid_chunks, mlp_pack (see pp_mlp_pack), warp_lean (see pp_warp_lean_begin)
 * pp_nerf_fwd and pp_nerf_bwd of one pass (and the two stages of a two-stage backward) must see the same option values.
 * Unknown names / out-of-range values are refused; pp_context_get_option(NULL, ...) reads the defaults. */
int pp_context_create(void** ctx);
int pp_context_destroy(void* ctx);
int pp_context_set_option(void* ctx, const char* name, int32_t value);
int pp_context_get_option(const void* ctx, const char* name, int32_t* value);

/* ---------------------------------------------------------------- MLPs on the matrix cores (fp32 MFMA).
 * rgbnet (voxurf_coarse.py:208-216, :1032-1033): 64(57)->128->128->128->3, sigmoid.
 * Parameter block layout (floats): W0[128*64] b0[128] W1[128*128] b1[128] W2[128*128] b2[128] W3[3*128] b3[3]
 * (W0 is the reference's [128,57] weight zero-padded to 64 columns).
 * acts[3][cap][128] keeps the hidden activations for the backward; acts = NULL: forward only (inference), nothing is kept -
 * accepted with the default split-precision forward kernel (option mlp_split bit 4), refused otherwise. */
#define PP_RGBNET_PARAMS (128 * 64 + 128 + 2 * (128 * 128 + 128) + 3 * 128 + 3)
int pp_rgbnet_fwd(const float* params, const float* feat, const int32_t* count, int32_t capacity, float* acts,
                  float* rgb, void* ctx, void* stream);
int pp_rgbnet_bwd(const float* params, const float* feat, const float* acts, const float* rgb,
                  const float* rgb_grad, const int32_t* count, int32_t capacity, float* scratch /*[3][cap][128] + 49152*/,
                  float* params_grad /*atomic +=*/, float* feat_grad, void* ctx /*pp_context or NULL*/, void* stream);

/* warp MLP (DeformedImplicitField, lib/deformation/deform_net.py:12-31, modules.py:43-124): 3->128x4->4 ReLU,
 * evaluated together with its input Jacobian in forward mode (row 0 primal, rows 1-3 tangents), which
 * replaces the reference's three autograd.grad(create_graph=True) passes (voxurf_coarse.py:972-984).
 * Parameter block: W0[128*3] b0[128] W1..W3[128*128]+b[128] each, W4[4*128] b4[4].
 * acts[4][cap*4][128] (NULL: forward only, as for pp_rgbnet_fwd; option mlp_split bit 1); out[M,4,4] (x out_range). */
#define PP_WARP_PARAMS (128 * 3 + 128 + 3 * (128 * 128 + 128) + 4 * 128 + 4)
int pp_warp_fwd(const float* params, const float* pts, const int32_t* count, int32_t capacity, float out_range,
                float* acts, float* out, void* ctx, void* stream);
int pp_warp_bwd(const float* params, const float* pts, const float* acts, const float* out_grad,
                const int32_t* count, int32_t capacity, float out_range, float* scratch /*[3][cap*4][128] + 49152*/,
                float* params_grad /*atomic +=*/, float* pts_grad /* += */, void* ctx /*pp_context or NULL*/,
                void* stream);

/* Workspace queries (floats) for the `acts` and `scratch` arguments of the MLP entry points at a sample capacity. */
int pp_rgbnet_workspace(int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats);
int pp_warp_workspace(int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats);
int pp_mlp_workspace(int32_t in_ld, int32_t n_gemm, int32_t capacity, int64_t* acts_floats, int64_t* scratch_floats);

/* Two-stage forms of the two backward chains above (layer-fused kernels only; option mlp_fused = 0 returns
 * PP_ERR_UNSUPPORTED): stage 1 = data gradients + thin-layer and bias gradients, leaves the hidden layers' output gradients
 * in `scratch`; stage 2 = the hidden layers' weight gradients from `scratch` and the stored activations.
 * pp_warp_bwd == pp_warp_bwd_data then pp_warp_bwd_weights (same for rgbnet); the split lets a caller time the kernels
 * separately, interleave other work, or put stage 2 on another stream.  Which stage produces the hidden layers' bias
 * gradients depends on the kernel stage 1 ran: stage 1 reports it in *stage2_host (a HOST int32, written before the call
 * returns) and the caller hands that value to stage 2 - stage 2 never re-derives it from its own context's options. */
int pp_warp_bwd_data(const float* params, const float* pts, const float* acts, const float* out_grad,
                     const int32_t* count, int32_t capacity, float out_range, float* scratch, float* params_grad,
                     float* pts_grad, int32_t* stage2_host, void* ctx, void* stream);
int pp_warp_bwd_weights(const float* acts, const float* scratch, const int32_t* count, int32_t capacity,
                        float* params_grad, int32_t stage2, void* ctx, void* stream);
int pp_rgbnet_bwd_data(const float* params, const float* acts, const float* rgb, const float* rgb_grad,
                       const int32_t* count, int32_t capacity, float* scratch, float* params_grad, float* feat_grad,
                       int32_t* stage2_host, void* ctx, void* stream);
int pp_rgbnet_bwd_weights(const float* feat, const float* acts, const float* scratch, const int32_t* count,
                          int32_t capacity, float* params_grad, int32_t stage2, void* ctx, void* stream);

/* Weight pack of the two object-branch MLPs (option mlp_pack, default 1).  The split-precision data-path kernels behind
 * pp_warp_fwd / pp_warp_bwd(_data) / pp_rgbnet_fwd / pp_rgbnet_bwd(_data) / pp_mlp_fwd / pp_mlp_bwd start by turning the
 * hidden layers' weights into fp16 hi | lo register images and by reducing their maxima and L1 norms - in every work-group of
 * every launch.  pp_mlp_pack does that work once (one small kernel on `stream`) into `pack` (pp_mlp_pack_workspace floats,
 * 16-byte aligned, caller-owned) and records `pack` and the two params pointers in `ctx` (required; either params pointer may be
 * NULL: that net is not packed).  A later call with THAT context and exactly THAT params pointer reads the pack (bit-identical
 * results); a call with ctx = NULL, with option mlp_pack = 0 or with any other params pointer derives everything itself, as
 * before.  The library cannot see writes to the parameters: whoever changes them (an optimiser step, a checkpoint load, a copy
 * into the buffer) must call pp_mlp_pack again, or pp_mlp_pack_invalidate, BEFORE the next MLP call with that context - on the
 * same stream as the write, so that the pack kernel reads the new values.  `pack` must stay alive, and unwritten by others,
 * until the record is replaced or invalidated and the kernels that read it are done.  With option mlp_pack = 0 (or no
 * split-precision kernel selected) pp_mlp_pack launches nothing and records nothing. */
int pp_mlp_pack_workspace(int64_t* pack_floats);
int pp_mlp_pack(const float* warp_params, const float* rgbnet_params, float* pack, void* ctx, void* stream);
int pp_mlp_pack_invalidate(void* ctx);
/* Head of a train step in ONE launch of independent work-group roles: pp_pose_fwd (same arguments, bit-identical w2c / c2w /
 * jac); step_dev[0..n_scalars) = step_scalars[0..n_scalars) - a HOST array of at most 32 floats, read during the call and handed
 * to the kernel by value, so that no copy sits in the stream (more than 32 are refused with PP_ERR_INVALID_ARG: upload them); zero_block[0..n_zero) = 0; and, with pack != NULL, pp_mlp_pack
 * (same pack, same record in `ctx`, which is then required; with option mlp_pack = 0 nothing is packed or recorded).  An earlier
 * record of `ctx` is dropped in every case. */
int pp_step_begin(const float* se3, const float* w2c_init, const int32_t* refine_mask, int32_t n_views, float* w2c,
                  float* c2w, float* jac, const float* step_scalars, int32_t n_scalars, float* step_dev,
                  float* zero_block, int32_t n_zero, const float* warp_params, const float* rgbnet_params, float* pack,
                  void* ctx, void* stream);

/* Lean scope of the warp net (option warp_lean, default 1).  Two of the per-sample blocks that the warp net's three kernels
 * exchange through `acts` and `scratch` can be rebuilt by their only reader, the weight-gradient kernel, from a few bytes:
 *   - the tangent rows of X0 (rows 4 s + 1 .. 4 s + 3 of acts slot 0) are  X0[4 s][n] > 0 ? W0[n][i] : 0;
 *   - Ybar3 (scratch slot 0) is  X3[4 s][n] > 0 ? sum_j W4[j][n] * out_range * out_grad[s][r][j] : 0.
 * pp_warp_lean_begin records `acts`, `scratch` and `params` in `ctx` (required); until pp_warp_lean_end(ctx), or the next
 * pp_warp_lean_begin, calls of pp_warp_fwd / pp_warp_bwd / pp_warp_bwd_data / pp_warp_bwd_weights with THAT context and exactly
 * THOSE acts (and scratch) pointers use the LEAN IMAGE of the two buffers:
 *   acts     slot 0: only the primal rows 4 s are written, the tangent rows are left untouched; slots 1 - 3 as always.
 *   scratch  slot 0: floats [0, 16 M) hold out_range * out_grad[s][r][j] at 16 s + 4 r + j, the rest of the slot is left
 *            untouched; slots 1 and 2 (Ybar2, Ybar1) as always.
 * out, pts_grad and everything else the data-path kernels write are bit-identical to the full form; the weight gradients of the
 * hidden layers agree with it to fp32 rounding.  All calls of one pass (forward, data gradients, weight gradients; one-shot or
 * staged) must be made inside one scope, with the recorded params: the weight-gradient stage reads W0 and W4 from that block.
 * A call with ctx = NULL, with another context or with any other acts / scratch pointer takes the full form, untouched, as does
 * every call after pp_warp_lean_end.  Only the split-precision kernels have a lean form: pp_warp_lean_begin records nothing
 * unless options mlp_fused = 1 and mlp_split bits 1, 2 and 16 are set, or when option warp_lean = 0.  Neither call launches
 * anything; ordered flushes (pp_ordered_attach) and the weight pack work inside a scope as outside. */
int pp_warp_lean_begin(const float* acts, const float* scratch, const float* params, void* ctx);
int pp_warp_lean_end(void* ctx);

/* Join scope of the weight gradients: the hidden layers' weight and bias gradients of BOTH nets in one launch.  Nothing but the
 * optimiser reads rgbnet's, and the warp net's chain - the same layer code - comes later on the same stream, so inside the scope
 *   - pp_rgbnet_bwd called with `ctx` runs its data-gradient kernel as always and, instead of launching its weight-gradient
 *     chain, RECORDS it in `ctx` (feat, acts, scratch, count, capacity, params_grad, stream) - if that chain would be the
 *     split-precision one (options mlp_fused = 1, mlp_split bits 8 and 16) and no ordered-flush workspace is attached; otherwise
 *     it launches it as always.  pp_rgbnet_bwd_weights and pp_mlp_bwd never defer.
 *   - the next pp_warp_bwd / pp_warp_bwd_weights with `ctx` launches ONE kernel for its own three products and the recorded
 *     three, if it runs the lean form of the split-precision chain (inside a pp_warp_lean_begin scope, for its buffers) with
 *     float atomics and is handed the SAME count pointer and stream as the record; otherwise it first launches the recorded
 *     chain on its own (on the recorded stream), exactly as pp_rgbnet_bwd would have.  Either way the record is cleared.
 * Between the two calls the recorded buffers must stay as they are and rgbnet's params_grad is incomplete.  The sums are the
 * same terms as in the two launches, shared out differently among the work-groups: results agree to fp32 rounding.
 * Work-groups (two per CU, or 2 x option mlp_wgs) are shared out 10 : 10 : 10 : 4 : 4 : 3 over the warp net's three layers,
 * rgbnet's two 128-wide layers and its input layer, rounded to nearest, the input layer taking the rest.
 * pp_wgrad_join_end closes the scope: a record nobody took is launched on its own (launch_pending = 1) or dropped
 * (launch_pending = 0: the pass failed, its gradients will not be used).  pp_wgrad_join_begin on an open scope ends it first,
 * with launch.  Neither is an option: outside a scope nothing changes. */
int pp_wgrad_join_begin(void* ctx);
int pp_wgrad_join_end(void* ctx, int32_t launch_pending);

/* ---------------------------------------------------------------- ordered gradient flushes: a bit-reproducible train step.
 * By default the parameter gradients of the object branch are accumulated with float atomics wherever several work-groups (or
 * lanes) contribute to one address: the hidden layers' weight and bias gradients of both MLPs (pp_warp_bwd, pp_rgbnet_bwd /
 * pp_mlp_bwd and their two-stage forms), their thin layers, sdf_ab_grad of the geometry backward and c2w_grad of the ray
 * backward.  Float addition is not associative, so the result depends on the order in which the hardware retires them.
 * With an ordered-flush workspace ATTACHED to a context, the MLP backward calls that are handed this context write per-work-group
 * partial sums with plain stores into `work` instead and add them up in ascending work-group order in a small reduction behind
 * each kernel (same stream), one writer per address; pp_geometry_bwd_priors_ordered and pp_raygen_select_bwd_ordered do the same
 * for the two calls that take no context otherwise (rows = work-groups / rays).  Guarantee: for one build of the library, equal
 * option values, equal shapes (capacity, n_rays, n_views, work-group counts) and the same device model, identical inputs give
 * bit-identical gradients.  NOT across different mlp_wgs values, builds or chips.  The surplus work-groups a persistent kernel
 * retires on the device when `count` is small are never read: the reduction derives the same active count from `count`.
 * Only the split-precision layer-fused kernels have this path: while a workspace is attached, the MLP backward entry points
 * refuse (PP_ERR_INVALID_ARG) option values that select other kernels (mlp_fused = 0, mlp_split without bits 2 / 8 / 16, generic
 * MLP shapes), rather than fall back to atomics.  The reported scalars (loss_out, tv_out) stay on atomics:
 * they feed no update.  The k0 scatter has its own ordered form (pp_k0_scatter_samples_sorted).
 * pp_ordered_workspace: bytes (a multiple of 16) for `work_groups` = the largest persistent grid the calls will use (the device's
 * compute-unit count, or option mlp_wgs when that is set; at least 16 are assumed), sample capacity and ray count; a pure host
 * function.  pp_ordered_attach records `work` (16-byte aligned, at least that many bytes, caller-owned, alive and untouched by
 * others while calls with this context are in flight) and the three sizes in `ctx`; calls that need more than was attached are
 * refused.  work = NULL detaches: back to atomics.  Order of magnitude: 2 x 2 x 256 x 64.5 KB = 66 MB on an MI355X. */
int pp_ordered_workspace(int32_t work_groups, int32_t capacity, int32_t n_rays, int64_t* bytes);
int pp_ordered_attach(void* ctx, void* work, int64_t work_bytes, int32_t work_groups, int32_t capacity, int32_t n_rays);
/* pp_geometry_fwd + pp_color_feat_fwd as work-group roles of ONE launch, for k0_dim = 12, pos_pe = 5, view_pe = 1: the geometry role
 * writes the normal columns and the zero padding of feat[M,64], the colour role the columns before them.  Every role runs the
 * stand-alone kernel's code: all outputs are bit-identical to the separate launches. */
int pp_geometry_color_feat_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                               const float* warp_out, const float* viewdirs, const int32_t* ray_id, const int32_t* count,
                               int32_t capacity, float inv_s, float* alpha, float* gradient, float* sdf_final,
                               float* sdf_deform, float* grad_deform, const float* k0_cl, const float* pe_w, float* feat,
                               void* stream);
/* pp_geometry_bwd_priors / pp_raygen_select_bwd (same arguments, same kernels, same results up to summation order) with
 * sdf_ab_grad (+=, required) / c2w_grad (overwritten, required) added up in work-group / ray order through the workspace attached
 * to `ctx` (required). */
int pp_geometry_bwd_priors_ordered(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts,
                                   const float* warp_out, const float* viewdirs, const int32_t* ray_id, const int32_t* count,
                                   int32_t capacity, float inv_s, const float* g_alpha, const float* g_gradient, float w_eikonal,
                                   float w_deform, float loss_scale, int32_t accumulate, float* warp_out_grad, float* pts_grad,
                                   float* viewdir_grad_s, float* sdf_ab_grad, float* loss_out, const float* batch_norm,
                                   void* ctx, void* stream);
int pp_raygen_select_bwd_ordered(const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays, const float* c2w,
                                 const float* intr, int32_t n_views, int32_t H, int32_t W, int32_t inverse_y,
                                 const float* rays_o, const float* rays_d, const float* t_min,
                                 const int32_t* ray_start, const float* pts_grad, const float* step,
                                 const float* viewdir_grad_s, const float* rays_o_grad, const float* rays_d_grad,
                                 const float* viewdirs_grad, const float* depth_grad, float* rays_o_grad_out,
                                 float* rays_d_grad_out, float* viewdirs_grad_out, float* c2w_grad, void* ctx, void* stream);

/* ---------------------------------------------------------------- losses: lib/losses.py:6-74 (object_losses),
 * forward values + gradients w.r.t. the render outputs in one pass.  loss_scale multiplies every gradient
 * (recon_scene.py:648 scales the object loss by 0.1).
 * loss_out[8] (atomic +=, caller zeroes): [0] mse, [1] entropy, [2] eikonal, [3] grad_deform, [4] sdf_correct,
 * [5] sdf_deform, [6] bce mask (unweighted scalars, as loss_scalars in the reference), [7] the WEIGHTED sum of the seven
 * (each kernel adds its share with its w_* arguments, loss_scale not applied): object_losses' `loss` without the TV term.
 * mask_sum[1] receives the batch's masked-pixel count.  g_rgb_marched is w.r.t. the CLAMPED rgb_marched
 * (pp_march_bwd applies the clamp mask).
 * batch_norm (device float[2], may be NULL): ray-sharded data parallelism.  The reference normalises the masked MSE by
 * the batch's masked-pixel count and the sample-level priors by the batch's sample count (lib/losses.py:6-29); with the
 * rays of ONE batch spread over W ranks and gradients averaged over ranks, batch_norm[0] = (sum over ranks of the
 * masked-pixel counts) / W and batch_norm[1] = (sum over ranks of the sample counts) / W make the sharded step equal the
 * union-batch step.  NULL = this call's own counts (single GPU). */
int pp_loss_rays(const float* rgb_marched, const float* alphainv_last, const float* cum_weights,
                 const float* target, const float* mask_px, float* mask_sum, int32_t n_rays, float w_main,
                 float w_entropy, float w_mask, float loss_scale, float* g_rgb_marched, float* g_alphainv_last,
                 float* g_cum_weights, float* loss_out, const float* batch_norm, void* stream);
/* pp_march_fwd -> pp_loss_rays -> pp_march_bwd in ONE launch, one wavefront per ray: the ray's composite, its loss terms and its
 * compositing backward in sequence, with the samples' values kept in registers (no nrm_in / normal_marched, no batch_norm: callers
 * that need them keep the separate calls).  sample_cap = an upper bound of the samples of one ray (ray_start[r + 1] - ray_start[r]);
 * the kernel holds 192: a larger sample_cap is refused with PP_ERR_INVALID_ARG before anything is launched - take the separate
 * calls then.  The bound is the CALLER'S promise: the kernel does not compare it with ray_start, and a ray that is longer all the
 * same is composited from its first 192 samples only (never indexed past them) - wrong outputs for that ray, no error.
 * Every output of the three calls is written; all are bit-identical to them except loss_out[0], [1], [6], [7] (+=),
 * whose sums are formed per work-group and added up in a fixed order by the last work-group to arrive: they differ from
 * pp_loss_rays' by summation order only, and are the same bits from call to call.
 * work: pp_march_loss_workspace bytes, 16-byte aligned, ZERO before the first call; every call leaves its first word zero again.
 * step_w, depth_acc, loss_out, g_depth_acc, g_weights, grad_rgb may be NULL (as in the separate calls). */
int pp_march_loss_workspace(int32_t n_rays, int32_t sample_cap, int64_t* bytes);
int pp_march_loss_bwd(const float* alpha, const float* rgb, const float* step_w, const int32_t* ray_start,
                      int32_t n_rays, int32_t sample_cap, float bg, float* weights, float* T, float* alphainv_last,
                      int32_t* i_end, float* rgb_marched, float* rgb_pre, float* cum_weights, float* depth_acc,
                      const float* target, const float* mask_px, float* mask_sum, float w_main, float w_entropy,
                      float w_mask, float loss_scale, float* g_rgb_marched, float* g_alphainv_last,
                      float* g_cum_weights, float* loss_out, const float* g_depth_acc, const float* g_weights,
                      float* grad_alpha, float* grad_rgb, void* work, int64_t work_bytes, void* stream);
/* g_gradient[M,3] is ACCUMULATED (+=); g_grad_deform[M,9], g_correction[M], g_sdf_deform[M] are written. */
int pp_loss_samples(const float* gradient, const float* grad_deform, const float* warp_out,
                    const float* sdf_deform, const int32_t* count, int32_t capacity, float w_eikonal,
                    float w_deform, float loss_scale, float* g_gradient, float* g_grad_deform,
                    float* g_correction, float* g_sdf_deform, float* loss_out, const float* batch_norm, void* stream);

/* ---------------------------------------------------------------- optimiser: lib/utils.py:82-198 (Adam, betas
 * (0.9,0.99)) fused with the k0 total-variation gradient (voxurf_coarse.py:443-456, :1298-1313; weight
 * tv_scale = loss_scale*weight_tv_k0/(3*numel)) and the gradient zero-fill, one streaming pass over the
 * channels-last grid.  Ping-pong parameter buffers (p_in read incl. neighbours, p_out written).
 * x-slab [x_begin,x_end) only (ZeRO-1 sharding across ranks); tv_out[1] += sum |diff| of the slab. */
int pp_grid_tv_adam_step(const float* p_in, float* p_out, float* grad, float* exp_avg, float* exp_avg_sq,
                         int32_t size_x, int32_t size_y, int32_t size_z, int32_t channels, int32_t x_begin,
                         int32_t x_end, float tv_scale, float grad_scale, float lr, float beta1, float beta2,
                         float eps, int32_t step, float* tv_out, void* ctx, void* stream);
/* Same pass for a SPARSE data gradient: `touched` (one byte per voxel, written by pp_k0_scatter_samples / _packed) tells
 * which voxels can hold a non-zero grad; for all others grad is neither read nor re-zeroed (96 of the 384 B/voxel).
 * Results are bit-identical to the dense pass as long as every non-zero grad voxel is marked.  `touched_clear` (the
 * map consumed by the PREVIOUS step, or NULL) is zeroed on the way; touched == NULL = dense behaviour. */
int pp_grid_tv_adam_step_sparse(const float* p_in, float* p_out, float* grad, float* exp_avg, float* exp_avg_sq,
                                int32_t size_x, int32_t size_y, int32_t size_z, int32_t channels, int32_t x_begin,
                                int32_t x_end, float tv_scale, float grad_scale, float lr, float beta1, float beta2,
                                float eps, int32_t step, float* tv_out, const uint8_t* touched, uint8_t* touched_clear,
                                void* ctx, void* stream);
/* pp_grid_tv_adam_step_sparse (touched / touched_clear may be NULL: the dense pass) that carries the end of the step as
 * work-group roles of the SAME launch - they read nothing the grid pass writes and run beside it instead of after it.
 * Always: pp_adam_flat(flat_*, grad_scale, step, zero_grad = 1).  se3 != NULL && se3_update: pp_adam_flat over the se3 block
 * [n_views*6], one segment with the learning rate pose_lr[0] (device).  sc != NULL (needs se3): ahead of the se3 update the
 * launch runs pp_raygen_select_bwd (c2w_grad and viewdir_grad_s only, no ray-level inputs or outputs) and pp_pose_bwd; the
 * last ray work-group to arrive does the pose part.  c2w_grad[n_views*12] and arrive[1] must be ZERO on entry and are zero
 * again when the launch ends (no per-step memset); with se3_update = 0 the launch stops at se3_grad = jac^T c2w_grad.
 * Every role runs the stand-alone kernel's code: outputs without float atomics are bit-identical to the separate launches. */
int pp_grid_tv_adam_step_tail(const float* p_in, float* p_out, float* grad, float* exp_avg, float* exp_avg_sq,
                              int32_t size_x, int32_t size_y, int32_t size_z, int32_t channels, int32_t x_begin,
                              int32_t x_end, float tv_scale, float grad_scale, float lr, float beta1, float beta2,
                              float eps, int32_t step, float* tv_out, const uint8_t* touched, uint8_t* touched_clear,
                              float* flat_p, float* flat_grad, float* flat_m, float* flat_v, int32_t flat_n,
                              const int32_t* flat_seg_end, const float* flat_seg_lr, int32_t flat_n_seg, float flat_beta1,
                              float flat_beta2, float flat_eps, float* se3, float* se3_grad, float* se3_m, float* se3_v,
                              int32_t n_views, const float* pose_lr, float pose_beta1, float pose_beta2, float pose_eps,
                              int32_t se3_update, const pp_scene* sc, const int32_t* ray_idx, int32_t n_rays,
                              const float* c2w, const float* intr, int32_t H, int32_t W, int32_t inverse_y,
                              const float* rays_o, const float* rays_d, const float* t_min, const int32_t* ray_start,
                              const float* pts_grad, const float* step_len, const float* viewdir_grad_s, const float* jac,
                              float* c2w_grad, int32_t* arrive, void* ctx, void* stream);
/* Flat Adam over a packed parameter buffer with per-segment learning rates: seg_end[n_seg], seg_lr[n_seg]. */
int pp_adam_flat(float* p, float* grad, float* exp_avg, float* exp_avg_sq, int32_t n, const int32_t* seg_end,
                 const float* seg_lr, int32_t n_seg, float grad_scale, float beta1, float beta2, float eps,
                 int32_t step, int32_t zero_grad, void* stream);
/* total_variation(v) value only (voxurf_coarse.py:1298-1313) on a channels-last grid: out[1] += sum|diff|. */
int pp_grid_tv_value(const float* p, int32_t size_x, int32_t size_y, int32_t size_z, int32_t channels, float* out,
                     void* stream);

/* Generic trilinear lookup on a channels-last grid [X,Y,Z,C] (C<=16): DenseGrid.forward (lib/grid.py:47-58; border=0
 * zeros padding) and grid_sampler's F.grid_sample path (lib/voxurf_coarse.py:540, lib/dvgo_ori.py:249-261; border=1).
 * pts[n,3] world coords -> out[n,C].  Backward: grid_grad_cl (atomic +=, may be NULL), pts_grad[n,3] (=, may be NULL). */
int pp_grid_sample_fwd(const pp_scene* sc, const float* grid_cl, int32_t channels, const float* pts, int32_t n_pts,
                       int32_t border, float* out, void* stream);
int pp_grid_sample_bwd(const pp_scene* sc, const float* grid_cl, int32_t channels, const float* pts, int32_t n_pts,
                       int32_t border, const float* out_grad, float* grid_grad_cl, float* pts_grad, void* stream);
/* total_variation backward (voxurf_coarse.py:1298-1313): grad += scale * g_scalar[0] * d(sum|diff|)/dp. */
int pp_grid_tv_grad(const float* p, int32_t size_x, int32_t size_y, int32_t size_z, int32_t channels, float scale,
                    const float* g_scalar, float* grad, void* stream);

/* Surface-point query (Voxurf.query_sdf_point_wocuda / _wodeform, voxurf_coarse.py:766-795, :809-837): first sign
 * change of the per-ray SDF samples and the linear zero crossing.  Compact mode: sdf[M] + ray_start[N+1] + step_k[M]
 * (out-of-bbox slots take the reference's default 1); dense mode (ray_start = step_k = NULL): sdf[N,S].
 * Outputs: pts[N,3] = o + d*(t_min + z0/|d|), mask[N] (uint8), optional sdf_dense[N,S], zval[N]. */
int pp_sdf_first_crossing(const float* sdf, const int32_t* ray_start, const int32_t* step_k, int32_t n_rays,
                          int32_t n_samples, float dist, const float* t_min, const float* rays_o,
                          const float* rays_d, float* sdf_dense, float* pts, uint8_t* mask, float* zval,
                          void* stream);

/* Backward of the DENSE-mode query above when its SDF row is the border-padded trilinear lookup of the raw template at
 * the dense sample positions p_k = o + d (t_min + dist (k + jitter) / |d|) (query_sdf_point_wocuda_wodeform,
 * voxurf_coarse.py:797-837; the reference differentiates it by autograd and recon_scene.py:336-340 back-propagates the
 * reprojection loss through it while at most two views are active).  sdf_grid [X,Y,Z]; sdf_dense[N,S] as returned by
 * the forward; jitter[N] or NULL (eval).  Upstream: g_pts[N,3] and / or g_sdf_dense[N,S] (either may be NULL).
 * Outputs (=): g_rays_o[N,3], g_rays_d[N,3] (incl. the |d| path), g_t_min[N]; t_min's own dependence on the ray
 * (slab test, :701-705) is the caller's to chain. */
int pp_sdf_crossing_dense_bwd(const pp_scene* sc, const float* sdf_grid, const float* rays_o, const float* rays_d,
                              const float* t_min, const float* jitter, int32_t n_rays, int32_t n_samples, float dist,
                              const float* sdf_dense, const float* g_pts, const float* g_sdf_dense, float* g_rays_o,
                              float* g_rays_d, float* g_t_min, void* stream);

/* ---------------------------------------------------------------- DVGO-surface operators of the reference's
 * extensions that the live loop never calls (SURVEY.md 2a "dead"), kept for API completeness:
 * raw2alpha{,_nonuni}{,_backward} (render_utils_kernel.cu:431-574; interval_v != NULL selects the per-point form),
 * maskcache_lookup (:374-424; world[X,Y,Z] uint8), sample_ndc_pts_on_rays (:245-293), sample_bg_pts_on_rays (:301-360),
 * adam_upd / masked_adam_upd / adam_upd_with_perlr (adam_upd_kernel.cu:8-133; mode 0/1/2),
 * total_variation_add_grad{,_new} (total_variation_kernel.cu:13-134; channels-last grids, mask_cl != NULL selects
 * the masked form), cumdist_thres (ub360_utils_kernel.cu:12-48). */
int pp_raw2alpha_fwd(const float* density, float shift, float interval, const float* interval_v, int32_t n,
                     float* exp_d, float* alpha, void* stream);
int pp_raw2alpha_bwd(const float* exp_d, const float* grad_back, float interval, const float* interval_v, int32_t n,
                     float* grad, void* stream);
int pp_maskcache_lookup(const uint8_t* world, const float* xyz, int32_t size_x, int32_t size_y, int32_t size_z,
                        float scale_x, float scale_y, float scale_z, float shift_x, float shift_y, float shift_z,
                        int32_t n, uint8_t* out, void* stream);
int pp_sample_ndc(const pp_scene* sc, const float* rays_o, const float* rays_d, int32_t n_rays, int32_t n_samples,
                  float* pts, uint8_t* mask_outbbox, void* stream);
int pp_sample_bg(const float* rays_o, const float* rays_d, const float* t_max, float bg_preserve, int32_t n_rays,
                 int32_t n_samples, float* pts, void* stream);
int pp_adam_upd(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* perlr, int32_t n,
                int32_t step, float beta1, float beta2, float lr, float eps, int32_t mode, void* stream);
/* pp_adam_upd (mode 0) over up to 32 small tensors of one optimiser group in ONE launch: the *_host arguments are HOST arrays of
 * n_tensors device pointers / sizes (copied into the kernel's arguments; nothing is dereferenced on the host).  Same arithmetic. */
int pp_adam_upd_multi(float* const* params_host, const float* const* grads_host, float* const* exp_avg_host,
                      float* const* exp_avg_sq_host, const int32_t* sizes_host, int32_t n_tensors, int32_t step, float beta1,
                      float beta2, float lr, float eps, void* stream);
int pp_tv_add_grad(const float* param_cl, float* grad_cl, const float* mask_cl, int32_t size_x, int32_t size_y,
                   int32_t size_z, int32_t channels, float wx, float wy, float wz, int32_t dense_mode, void* stream);
int pp_cumdist_thres(const float* dist, float thres, int32_t n_rays, int32_t n_pts, uint8_t* mask, void* stream);

/* ---------------------------------------------------------------- DirectVoxGO twin (lib/dvgo_ori.py:289-379).
 * Generic feature builder: [k0 (channels k0_skip..C) | xyz PE | view PE | optional normal], row stride ld (multiple of
 * 32), un-weighted encodings when pe_w == NULL, sel[M] (uint8, optional) = weights > fast_color_thres mask, optional
 * k0_raw[M,C] copy of the interpolated features (k0_diffuse for rgbnet_direct=False). */
int pp_feat_generic_fwd(const pp_scene* sc, const float* k0_cl, const float* pts, const float* viewdirs,
                        const int32_t* ray_id, const float* gradient, const float* pe_w, const uint8_t* sel,
                        int32_t k0_skip, int32_t ld, const int32_t* count, int32_t capacity, float* feat,
                        float* k0_raw, void* stream);
int pp_feat_generic_bwd_k0(const pp_scene* sc, const float* pts, const uint8_t* sel, int32_t k0_skip, int32_t ld,
                           const int32_t* count, int32_t capacity, const float* feat_grad,
                           const float* k0_raw_grad, float* k0_grad_cl, void* stream);
/* Generic ReLU MLP in_ld -> 128 x n_gemm -> 3 + sigmoid on the matrix cores.  Parameter block:
 * W0[128*in_ld] b0[128] | (W[128*128] b[128]) x (n_gemm-1) | Wout[3*128] bout[3].  logit_add[M,ld] (optional) is
 * added to the logits before the sigmoid (k0_diffuse, dvgo_ori.py:359).  acts[n_gemm][cap][128];
 * scratch [3][cap][128] + 16384. */
int pp_mlp_fwd(const float* params, const float* feat, int32_t in_ld, int32_t n_gemm, const int32_t* count,
               int32_t capacity, const float* logit_add, int32_t logit_add_ld, float* acts, float* out,
               void* ctx, void* stream);
int pp_mlp_bwd(const float* params, const float* feat, int32_t in_ld, int32_t n_gemm, const float* acts,
               const float* out, const float* out_grad, const int32_t* count, int32_t capacity, float* scratch,
               float* params_grad, float* feat_grad, float* logit_add_grad, int32_t logit_add_ld, void* ctx,
               void* stream);
/* cumprod_exclusive(clamp_min(1-alpha,1e-10)) compositing without early stop (dvgo_ori.py:478-489): weights[M], T[M],
 * alphainv_last[N], rgb_acc[N,3] = sum w*rgb (un-clamped, bg not added), cum_weights[N], depth_acc[N] = sum w*step_w.
 * The backward is pp_march_bwd. */
int pp_march_dvgo_fwd(const float* alpha, const float* rgb, const float* step_w, const int32_t* ray_start,
                      int32_t n_rays, float* weights, float* T, float* alphainv_last, int32_t* i_end,
                      float* rgb_acc, float* cum_weights, float* depth_acc, void* stream);

/* ---------------------------------------------------------------- scene branch: NeRF MLP + compositing
 * (lib/bg_nerf/source/models/frequency_nerf.py).  Replaces NeRF.forward_samples (:268-288 -> compute_raw_density :149-170,
 * forward :172-227, positional_encoding :239-266 with FrequencyEmbedder :42-69) and NeRF.composite (:290-343) for the
 * default architecture (default_config.py:90-105): L_3D = 10, L_view = 4 with raw coordinates, 8 x 256 feature layers,
 * skip at 4, softplus density, 283 -> 128 -> 3 colour head.
 *
 * Parameter block (floats), offsets from pp_nerf_layout(offsets[23]) = {W0,b0,...,W7,b7,wd,bd,R0,br0,R1,br1,total}:
 *   W0[256][64] (63 used) | W1..W3[256][256] | W4[256][320] (features 0..255, encoding 256..318) | W5,W6 |
 *   wd[256] W7[256][256] | bd b7[256] = the reference's last layer [257][256] / [257] stored contiguously (row 0 = density) |
 *   R0[128][288] (features 0..255, view encoding 256..282) | R1[3][128].
 * Rays: center[R,3], ray[R,3] (un-normalised), depth[R,S]; sample m = r * S + s.  bands[14] (device) = BARF's coarse-to-fine
 * weights of the 10 point bands then the 4 view bands (ones without a schedule).  count: device int32 holding R * S.
 * Workspaces in floats from pp_nerf_workspace(R * S, R, &acts, &scratch).
 * Arithmetic: fp32 operands and accumulation; the forward / data-gradient / weight-gradient matrix products are evaluated as
 * three fp16 products per fp32 product (error against fp64 equal to the fp32 matrix instructions'); option
 * nerf_split = 0 (of the context handed to the call) selects the fp32 matrix instructions instead. */
int pp_nerf_layout(int64_t* offsets);
int pp_nerf_workspace(int64_t n_samples, int64_t n_rays, int64_t* acts_floats, int64_t* scratch_floats);
int pp_nerf_fwd(const float* params, const float* center, const float* ray, const float* depth, const float* bands,
                const int32_t* count, int32_t n_rays, int32_t n_samples, float* acts, float* rgb_samples,
                float* density_samples, void* ctx, void* stream);
/* Backward of pp_nerf_fwd: params_grad is ACCUMULATED into (zero it first); g_center[R,3] and g_ray[R,3] are overwritten
 * (g_ray holds the point and view-direction paths; the compositing path is pp_nerf_composite_bwd's g_ray). */
int pp_nerf_bwd(const float* params, const float* ray, const float* depth, const int32_t* count, int32_t n_rays,
                int32_t n_samples, const float* acts, const float* rgb_samples,
                const float* g_rgb_samples, const float* g_density_samples, float* scratch, float* params_grad,
                float* g_center, float* g_ray, void* ctx, void* stream);
/* Backward of pp_nerf_fwd with respect to the rays only (frozen parameters: test-time pose refinement): the launches of
 * pp_nerf_bwd without its nine weight-gradient products, on the fused route and on the layer-by-layer route of either arithmetic.  g_center and
 * g_ray are bit-identical to pp_nerf_bwd's on the same inputs; no parameter gradient exists (the two thin heads' sums, whose
 * kernels also record operand maxima the later kernels read, are added into a part of `scratch` that nothing reads before
 * the data-gradient kernels of either route overwrite it).  Same workspaces as pp_nerf_bwd (pp_nerf_workspace is unchanged).  A workspace attached with
 * pp_nerf_ordered_attach is neither used nor refused: nothing is flushed. */
int pp_nerf_bwd_input(const float* params, const float* ray, const float* depth, const int32_t* count, int32_t n_rays,
                      int32_t n_samples, const float* acts, const float* rgb_samples, const float* g_rgb_samples,
                      const float* g_density_samples, float* scratch, float* g_center, float* g_ray, void* ctx, void* stream);
/* Forward pass that keeps no activations (whole views, validation images, novel-view sequences): pp_nerf_fwd's arguments with
 * `work` (pp_nerf_infer_workspace floats) in place of `acts`; rgb_samples[M,3] and density_samples[M] are bit-identical to
 * pp_nerf_fwd's on the same inputs and context (same operand scales, same accumulation, same summation order).  No layer
 * output and no ReLU mask is written to memory: work = 224 floats per sample (encoded points 64, view encoding 32, the colour
 * head's hidden layer 128) + the operand-maximum slots and the packed weight stream (573 504 floats, independent of the sample
 * count), against pp_nerf_workspace's 2337 floats + 256 mask bytes per sample.  Only the fused route (the default) has this form: a context
 * with nerf_split != 1 or nerf_chain != 3 is refused with PP_ERR_INVALID_ARG (use
 * pp_nerf_fwd there).  pp_nerf_bwd cannot follow this call. */
int pp_nerf_infer_workspace(int64_t n_samples, int64_t n_rays, int64_t* work_floats);
int pp_nerf_infer(const float* params, const float* center, const float* ray, const float* depth, const float* bands,
                  const int32_t* count, int32_t n_rays, int32_t n_samples, float* work, float* rgb_samples,
                  float* density_samples, void* ctx, void* stream);
/* composite (:290-343): rgb[R,3] (+ 1 - opacity when white_bg), depth[R], opacity[R], weights[R,S], all_cumulated[R]
 * (= T at the second-to-last sample), rgb_var[R], depth_var[R] (the two variances are forward-only outputs). */
int pp_nerf_composite_fwd(const float* rgb_samples, const float* density_samples, const float* depth, const float* ray,
                          int32_t n_rays, int32_t n_samples, int32_t white_bg, float* rgb, float* depth_out, float* opacity,
                          float* weights, float* all_cumulated, float* rgb_var, float* depth_var, void* stream);
int pp_nerf_composite_bwd(const float* rgb_samples, const float* density_samples, const float* depth, const float* ray,
                          const float* weights, int32_t n_rays, int32_t n_samples, int32_t white_bg, const float* g_rgb,
                          const float* g_depth, const float* g_opacity, const float* g_weights, float* g_rgb_samples,
                          float* g_density_samples, float* g_ray, void* stream);

/* BARF coarse-to-fine band weights on the device (frequency_nerf.py:250-253): bands[l_3d + l_view] from the device scalar
 * `progress` - the schedule costs one launch and no host synchronisation.  width = end - start of opt.barf_c2f, formed in double
 * by the caller and rounded once (what torch does with the Python scalar). */
int pp_nerf_band_weights(const float* progress, float start, float width, int32_t l_3d, int32_t l_view, float* bands, void* stream);
/* Photometric loss of the scene branch (base_losses.py:155-156, :304-307): loss[0] = weight * huber_loss(pred, label, delta,
 * 'mean') over n floats, g_pred[n] = d loss / d pred.  Deterministic (one work-group, fixed summation order). */
int pp_nerf_huber_loss(const float* pred, const float* label, int32_t n, float delta, float weight, float* loss, float* g_pred,
                       void* stream);
/* The two per-iteration pieces of test-time pose refinement (eval.py:838-858) beside the network (csrc/pp_pose_refine.hip).
 * pp_nerf_rays_select: the rays and targets of n_rays chosen pixels of ONE view (utils/camera.py:347-416 + the target gather of
 * eval.py:851-852).  ray_idx[n_rays] in [0, H * W) indexes the row-major pixels (the caller guarantees the range; an index outside it is clamped, so no read leaves the image); pixel centre
 * (idx % W + 0.5, idx / W + 0.5); dir_cam = K^-1 [x, y, 1] by the closed form for an UPPER-TRIANGULAR K[3,3] with K[2][2] = 1
 * (skew K[0][1] included; the caller checks the form); ray = R dir_cam (un-normalised) and center = t of c2w[3,4] = [R | t];
 * target = image[H,W,3] at the pixel.  c2w, K and image are device memory.  Outputs [n_rays,3] each, overwritten.
 * pp_nerf_mse_loss: loss[0] = weight * mean((pred - label)^2) over n floats (F.mse_loss, eval.py:853), g_pred[n] its gradient.
 * Deterministic (one work-group, strided partial sums, then a tree with fixed pairs, as pp_nerf_huber_loss). */
int pp_nerf_rays_select(const float* c2w, const float* K, const int32_t* ray_idx, int32_t n_rays, int32_t H, int32_t W,
                        const float* image, float* center, float* ray, float* dir_cam, float* target, void* stream);
int pp_nerf_mse_loss(const float* pred, const float* label, int32_t n, float weight, float* loss, float* g_pred, void* stream);

/* SPARF correspondence loss on rendered depths (lib/bg_nerf/source/training/core/corres_loss.py:93-222, the re-projection of
 * batched_geometry_utils.py:199-228 and the Huber term of base_losses.py:197-224), forward and backward in one launch.
 * depth0 / depth1 = the coarse / fine pass's rendered depths of the matched rows, [self n_pairs | other n_pairs] each (depth1 =
 * NULL: one pass); pix_self, pix_other [n_pairs,2], conf [n_pairs]; K_self, K_other [3,3]; w2c_self, w2c_other [3,4] - all
 * read from device memory.  Both directions of every pass, each normalised by its count of valid rows + 1e-6 (the detached
 * pixel / depth re-projection filters), summed, / 2 (one pass) or / 4, times `weight`, into loss[0].  g_depth0 / g_depth1
 * [2 n_pairs] = d loss / d depth (overwritten); g_w2c [2,3,4] = d loss / d (w2c_self, w2c_other) through T_self2other and
 * its inverse (overwritten).  Deterministic (one work-group, fixed summation order); no valid row gives 0 everywhere. */
int pp_nerf_corres_loss(const float* depth0, const float* depth1, int32_t n_pairs, const float* pix_self, const float* pix_other,
                        const float* conf, const float* K_self, const float* K_other, const float* w2c_self,
                        const float* w2c_other, int32_t pixel_check, float pixel_thresh, int32_t depth_check, float depth_thresh,
                        float weight, float* loss, float* g_depth0, float* g_depth1, float* g_w2c, void* stream);
/* Pose gradient of the matched rows: rows [0, n_pairs) of g_center / g_ray / dir_cam [2 n_pairs, 3] are view view_self's,
 * rows [n_pairs, 2 n_pairs) view view_other's.  g_c2w[v] += [sum g_ray (x) dir_cam | sum g_center] + g_w2c (may be NULL)
 * [2,3,4] moved onto c2w through w2c = [R^T | -R^T t] with w2c [n_views,3,4].  g_c2w [n_views,3,4] is ACCUMULATED into, so
 * it composes with the photometric rows' gradient before pp_pose_bwd.  Deterministic (one work-group). */
int pp_nerf_pair_pose_bwd(const float* g_center, const float* g_ray, const float* dir_cam, int32_t n_pairs, const float* w2c,
                          const float* g_w2c, int32_t n_views, int32_t view_self, int32_t view_other, float* g_c2w,
                          void* stream);

/* ---------------------------------------------------------------- object branch: reprojection + near-surface pose terms
 * lib/recon_scene.py:321-369 (get_project_error) as a second small ray batch of the object branch.  Row r: own view own[r],
 * other view other[r] (int32), pixel pix[r] (x, y) in the own view, matched pixel match[r] in the other view, confidence
 * conf[r].  Every per-row array below holds `capacity` rows; rows at or beyond n_rows (and rows whose view index lies outside
 * [0, n_views)) are never read from the row inputs and contribute nothing: their per-row outputs are written as zeros, their
 * rays miss the box.  intr [n_views,4] (fx, fy, cx, cy), c2w / w2c [n_views,3,4].
 * pp_reproj_rays: cam = [(x - cx) / fx, (y - cy) / fy, 1] (no half-pixel shift, inverse_y), rays_d = viewdirs =
 * normalize(R_c2w cam), rays_o = t_c2w of the own view (recon_scene.py:93-113 with mode 'no_center'). */
int pp_reproj_rays(const pp_scene* sc, const int32_t* own, const float* pix, int32_t n_rows, int32_t capacity, const float* intr,
                   const float* c2w, int32_t n_views, float* rays_o, float* rays_d, float* viewdirs, void* stream);
/* Dense sample positions of the zero-crossing query (Voxurf.sample_ray_ori, voxurf_coarse.py:697-719, without the in-box
 * compaction): pts[r, k] = o + d (t_min + stepsize voxel_size (k + jitter[r]) / |d|), k < sc->n_samples; pts [n_rays, S, 3]. */
int pp_reproj_dense_pts(const pp_scene* sc, const float* rays_o, const float* rays_d, const float* t_min, const float* jitter,
                        int32_t n_rays, float* pts, void* stream);
/* Loss and every gradient that does not need the renderer.  render = 0: the surface point p [capacity,3] and the hit flag hit
 * [capacity] (uint8) are inputs (pp_sdf_first_crossing); render = 1 (p = hit = NULL): depth = t_min[r] + acc[r] with acc = the
 * ray's sum of weight x step (pp_march_fwd's depth), hit = acc > 0, p = o + d depth.
 *   near  = sum_r max(dist_r - half_diagonal, 0) [conf > 0], dist = distance of `centre` to the half-line o + t d, t >= 0
 *   q = R_w2c p + t_w2c of the OTHER view; behind = q_z < nl, then q := (nl, nl, nl) without gradient; (u, v) = K q / q_z
 *   e = |(u, v) - match|; valid = !behind && hit && (e <= pixel_thre, when pixel_check); err = sum valid conf huber_1(e) /
 *   (sum valid + 1e-6)
 * terms[3] = (err, near, sum valid), overwritten.  The gradients of scale (w_near near + w_proj err), all overwritten:
 * g_p [capacity,3]; g_depth [capacity] = g_p . d (render; 0 otherwise); g_o / g_d [capacity,3] = the direct gradient on the ray
 * (near term, and with render = 1 the ray's explicit share of p: g_o += g_p, g_d += depth g_p); g_w2c [n_views,3,4] = the direct
 * gradient on the other views' w2c.  One work-group, fixed summation order (strided per-thread partials, then a tree), no
 * atomics: identical inputs give identical bits. */
int pp_reproj_loss(int32_t render, int32_t n_rows, int32_t capacity, const int32_t* other, const float* match, const float* conf,
                   const float* rays_o, const float* rays_d, const float* p, const uint8_t* hit, const float* t_min,
                   const float* acc, const float* intr, const float* w2c, int32_t n_views, float centre_x, float centre_y,
                   float centre_z, float half_diagonal, float nl, int32_t pixel_check, float pixel_thre, float w_near,
                   float w_proj, float scale, float* terms, float* g_p, float* g_depth, float* g_o, float* g_d, float* g_w2c,
                   void* stream);
/* Own-view pose gradient: per-row ray gradients g_o, g_d, g_viewdirs (may be NULL) [capacity,3] and g_t_min (may be NULL)
 * [capacity] - chained through the slab test of the sampler (voxurf_coarse.py:701-705, differentiated w.r.t. rays_o / rays_d
 * [capacity,3]) - go through the direction normalisation and c2w of the own view and are summed per view; g_w2c (may be NULL)
 * [n_views,3,4] is moved onto c2w through w2c = [R^T | -R^T t] as pp_nerf_pair_pose_bwd does.  g_c2w [n_views,3,4] is
 * OVERWRITTEN (feed it to pp_pose_bwd).  One work-group per view, fixed summation order, no atomics. */
int pp_reproj_pose_fold(const pp_scene* sc, const int32_t* own, const float* pix, int32_t n_rows, const float* intr,
                        const float* c2w, const float* w2c, int32_t n_views, const float* rays_o, const float* rays_d,
                        const float* g_o, const float* g_d, const float* g_viewdirs, const float* g_t_min, const float* g_w2c,
                        float* g_c2w, void* stream);

/* ---------------------------------------------------------------- object branch: surface-projection feature loss
 * lib/recon_scene.py:371-439 (get_project_feature_loss) for ONE view pair (view_i, view_j), inverse_y without flips.  Query A
 * (rays_o, rays_d, t_min, acc; the caller's differentiable render of R rays) gives p = o + d (t_min + acc), hit = acc > 0.
 * Every per-row array holds `capacity` rows; rows at or beyond n_rows are never read and get zeros.
 * pp_featproj_reproject: q = w2c[view_j] p; q_z < nl: q := (nl, nl, nl); pix_ref [capacity,2] = K_j q / q_z
 * (lib/common.py:450-465), own_ref [capacity] int32 = view_j - the inputs of pp_reproj_rays for query B.  Rows from n_rows on get
 * own_ref = -1 (no view: pp_reproj_rays gives them a ray that misses the box) and pixel (0, 0).  nl must be positive. */
int pp_featproj_reproject(int32_t n_rows, int32_t capacity, int32_t view_j, const float* rays_o, const float* rays_d,
                          const float* t_min, const float* acc, const float* intr, const float* w2c, int32_t n_views, float nl,
                          int32_t* own_ref, float* pix_ref, void* stream);
/* The loss and every gradient up to the renderer.  ref_*: query B (forward only), p_ref and hit_ref as above.
 *   q_v = w2c[v] p for v = view_i, view_j with the near-plane replacement (which stops that view's gradient of the row);
 *   (x, y)_v = (2 u / (W - 1) - 1, 2 v / (H - 1) - 1), (u, v) = K_v q / q_z                            (lib/common.py:468-492)
 *   valid = |p - p_ref| < 2 voxel_size && hit && hit_ref && max(|x|, |y|) <= 1 in both views
 *   per layer l: a, b = bilinear samples (grid_sample, align_corners, zero padding) of feat_l[view_i], feat_l[view_j] at the
 *   two positions; cos = (a / max(|a|, 1e-8)) . (b / max(|b|, 1e-8)) with torch.nn.functional.cosine_similarity's derivative
 *   L = sum_l (1 - sum_valid cos / n_valid); without a valid row L and every gradient are exactly 0 (the reference: NaN).
 * feat0..feat3: n_layers <= 4 maps, channels-last [n_views,h,w,C] fp32 (unused ones NULL); layer_dims: HOST array
 * [n_layers,3] int32 of (C, h, w), 1 <= C <= 512, h, w >= 2.
 * Outputs, all overwritten: terms [6] = (L, n_valid, sum_valid cos of layers 0..3); valid [capacity] uint8; cosv
 * [n_layers,capacity] (0 where not valid); g_q [capacity,6] = the gradient of scale weight L on (q_i, q_j); g_depth [capacity],
 * g_o / g_d [capacity,3] = its gradient on query A's depth and on the ray's explicit share of p (g_o = g_p, g_d = depth g_p);
 * g_w2c [n_views,3,4] = the direct gradient on w2c (zero but for view_i and view_j).  Three launches: one work-group for the
 * flags and n_valid, one wavefront per row with lanes across channels, one work-group for the sums over rows.  Fixed summation
 * order, no atomics: identical inputs give identical bits. */
int pp_featproj_loss(int32_t n_rows, int32_t capacity, int32_t view_i, int32_t view_j, const float* rays_o, const float* rays_d,
                     const float* t_min, const float* acc, const float* ref_rays_o, const float* ref_rays_d,
                     const float* ref_t_min, const float* ref_acc, const float* intr, const float* w2c, int32_t n_views, float nl,
                     float voxel_size, int32_t H, int32_t W, int32_t n_layers, const float* feat0, const float* feat1,
                     const float* feat2, const float* feat3, const int32_t* layer_dims, float weight, float scale, float* terms,
                     uint8_t* valid, float* cosv, float* g_q, float* g_depth, float* g_o, float* g_d, float* g_w2c, void* stream);

/* ---------------------------------------------------------------- scene branch: ordered weight-gradient flush
 * The nine weight-gradient products of pp_nerf_bwd end in float atomics: up to 512 work-groups (row splits x 128 x 128 output
 * blocks) add their block to params_grad, in the order the hardware retires them.  With a workspace ATTACHED to the context
 * handed to pp_nerf_bwd, every work-group instead stores its scaled block and its 128 bias sums with plain stores into its own
 * slot, and a reduction launched behind each product on the same stream adds the slots of an output block in a fixed order (a
 * function of the row count alone) and adds the total to params_grad, one writer per address.  The row splits that receive no
 * rows return before the flush; the reduction derives the same active count from `count` on the device and never reads their
 * slots.  Every other sum of pp_nerf_fwd / pp_nerf_bwd is order-free already, so for one build, equal option values, equal
 * shapes and the same device model identical inputs then give bit-identical params_grad, g_center and g_ray.
 * pp_nerf_ordered_workspace: bytes of the workspace, a pure host function: 512 slots x (64 KB + 512 B) whatever the shapes (one
 * launch's worth serves all nine products of a pass and any number of networks whose calls share a stream).
 * pp_nerf_ordered_attach records `work` (16-byte aligned, at least that many bytes, caller-owned, alive and untouched by
 * others while calls with this context are in flight) in `ctx`; work = NULL detaches: back to atomics.  Only the split-precision
 * kernel has this flush: while a workspace is attached, pp_nerf_bwd with nerf_split = 0 is refused (PP_ERR_INVALID_ARG) rather
 * than run on atomics. */
int pp_nerf_ordered_workspace(int64_t* bytes);
int pp_nerf_ordered_attach(void* ctx, void* work, int64_t work_bytes);
/* The two sums of a joint step that the host otherwise forms with library reductions of unspecified order.
 * pp_nerf_c2w_fold: g_c2w[v] = [sum_n g_ray[v][n] (x) dir_cam[v][n] | sum_n g_center[v][n]] for v < n_views over g_ray, g_center,
 * dir_cam [n_views, n_rays, 3]; rows n_views .. n_views_total - 1 of g_c2w [n_views_total, 3, 4] receive zeros (overwritten).
 * One work-group per view: a thread adds its rays in ascending order, the threads fold by a tree with fixed pairs.
 * pp_nerf_sample_pdf: inverse-transform samples of the coarse weights merged with the coarse depths (renderer.py:702-738 and
 * the cat + sort of :596-600): weights, depth [n_rays, n_samples]; grid [n_fine + 1], or [n_rays, n_fine + 1] when grid_per_ray;
 * u_j = (grid_j + grid_j+1) / 2; pdf = w / (sum w + 1e-6), cdf its prefix sum (fixed order), the search of searchsorted(right =
 * True), t = (u - cdf_lo) / (cdf_hi - cdf_lo + 1e-8) between the bin edges linspace(depth_min, depth_max, n_samples + 1);
 * depth_out [n_rays, n_samples + n_fine] ascending.  One wavefront per ray; n_samples, n_fine <= 256. */
int pp_nerf_c2w_fold(const float* g_ray, const float* g_center, const float* dir_cam, int32_t n_views, int32_t n_rays,
                     int32_t n_views_total, float* g_c2w, void* stream);
int pp_nerf_sample_pdf(const float* weights, const float* depth, const float* grid, int32_t grid_per_ray, int32_t n_rays,
                       int32_t n_samples, int32_t n_fine, float depth_min, float depth_max, float* depth_out, void* stream);

/* ---------------------------------------------------------------- mesh extraction: marching cubes
 * lib/dvgo_ori.py:695-703 calls mcubes.marching_cubes(u, threshold) on a host lattice; here u [X,Y,Z] (fp32, C order, the
 * layout extract_fields fills) stays on the device and the result is an indexed mesh with shared vertices in lattice (index)
 * coordinates: vertices [n_vertices,3] fp32, triangles [n_triangles,3] int32 vertex ids.
 *   - a corner is BELOW iff u < threshold (fp32 compare); a lattice edge is ACTIVE iff exactly one endpoint is below; it is
 *     owned by its lower endpoint p0 and its axis a (0 x, 1 y, 2 z);
 *   - every active edge carries one vertex: t = (threshold - u[p0]) / (u[p1] - u[p0]) in fp32 (0 <= t <= 1), coordinate a is
 *     float(p0[a]) + t, the other two are the integers of p0;
 *   - canonical order, no atomics: the vertex id is the rank of its edge among the active edges in the order
 *     3 (x Y Z + y Z + z) + a; triangles are ordered by cell in C order over (X-1, Y-1, Z-1), then by table row order: the
 *     output is bit-reproducible;
 *   - winding: the geometric normal (v1 - v0) x (v2 - v0) points toward DECREASING u (for u = -sdf: outward);
 *   - non-finite field values are the caller's problem (a NaN corner counts as not below; its edges interpolate to NaN).
 * Case table (pp_mc_table, a pure host function: table [256*16] int32 on the HOST): corner c of a cell sits at offset
 * (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's low corner and bit c of the case index is set iff that corner is below;
 * edge e in 0..11 runs along axis a = e >> 2, and with j = e & 3 its lower endpoint sits at the offset whose two OTHER
 * coordinates, in ascending axis order, are (j & 1, j >> 1) (edge 0..3: x edges at (y,z) = (0,0) (1,0) (0,1) (1,1); 4..7: y
 * edges at (x,z) likewise; 8..11: z edges at (x,y) likewise).  Row `case` holds at most 5 triangles as triples of edge ids,
 * terminated by -1 (tools/gen_mc_table.py generates it; tests/test_mesh_host.py checks its properties exhaustively).
 * pp_mc_workspace (pure host function): bytes of `work` for a lattice - one flag byte and one int32 vertex base per point
 * (padded to whole 1024-point tiles) plus 8 bytes per tile, about 5 X Y Z.
 * pp_mc_count classifies the lattice into `work` and writes counts[2] (DEVICE) = (vertices, triangles); a triangle total
 * above 2^31 - 1 is reported as -1.  pp_mc_emit, given the SAME u, sizes, threshold and work, ordered behind pp_mc_count,
 * writes rows [0, n_vertices) and [0, n_triangles) - the counted rows when handed the counts - and nothing past them.
 * `work` is 16-byte aligned.  All four refuse, before any GPU call: null pointers, a dimension below 2, 3 X Y Z >= 2^31
 * (PP_ERR_UNSUPPORTED: vertex ids are 32-bit), a workspace that is too small. */
int pp_mc_table(int32_t* table_host);
int pp_mc_workspace(int32_t X, int32_t Y, int32_t Z, int64_t* bytes);
int pp_mc_count(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, void* work, int64_t work_bytes,
                int32_t* counts, void* stream);
int pp_mc_emit(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, void* work, int64_t work_bytes,
               float* vertices, int32_t n_vertices, int32_t* triangles, int32_t n_triangles, void* stream);

/* Vertex attributes of an extracted mesh (csrc/pp_mesh_color.hip): the render path's colour stage with every
 * vertex seen head-on.  pts [n,3] in model coordinates; warp_out [n,4,4] = pp_warp_fwd's rows for these points, or NULL for the
 * plain template (use_deform=False).  g = d sdf / d p is pp_geometry_fwd's `gradient` (pp_geometry_plain_fwd's without
 * warp_out); normal [n,3] = g / (|g| + 1e-5); feat [n,64] = the row pp_rgbnet_fwd reads, as pp_color_feat_fwd lays it out, with
 * the view embedding formed from viewdir = -normal: [k0 (12) | xyz PE (33) | view PE (9) | normal (3) | 0 (7)].  pe_w [6] as
 * for pp_color_feat_fwd.  One forward-only launch: no atomics, no workspace, rows from n on are not written; n = 0 launches
 * nothing.  Only k0_dim = 12, pos_pe = 5, view_pe = 1 (PP_ERR_UNSUPPORTED otherwise). */
int pp_vertex_feat(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* k0_cl, const float* pts,
                   const float* warp_out, const float* pe_w, int32_t n, float* normal, float* feat, void* stream);

/* Connected components of an indexed mesh (csrc/pp_mesh_components.hip): triangles [n_triangles,3] int32 over
 * n_vertices vertices; two vertices are connected when some triangle contains both (a shared vertex is enough).
 *   labels [n_vertices] int32 = the smallest vertex index of the vertex's component; -1 for a vertex no triangle references.
 * That is the unique fixpoint of "hook to the smaller label, then shortcut", reached in rounds of two launches (hook: one thread
 * per triangle, atomicMin; jump: one thread per vertex, a bounded walk of its own chain).  A round reads only what the round
 * before left and combines it with minima, so labels AND the number of rounds are pure functions of the mesh.  No launch waits
 * for another work-group; the host decides when to stop.
 * pp_cc_workspace (pure host function): bytes of `work` - two int32 arrays of n_vertices, each rounded up to 256 bytes.
 * pp_cc_rounds runs rounds first_round .. first_round + n_rounds - 1 (first_round = 0 initialises labels and work first;
 *   1 <= n_rounds <= 1024) and sets changed[k] (DEVICE int32 [n_rounds], cleared by the call, raised by plain stores) to 1 iff
 *   the k-th of them changed a label.  A round that changes nothing is the fixpoint, and so is every round after it.  `labels`
 *   and `work` carry the state from call to call.  n_triangles = 0 leaves every label at -1.
 * pp_cc_count: vertex_counts / triangle_counts [n_vertices] int32 (cleared by the call), indexed BY ROOT: the referenced
 *   vertices / the triangles of the component whose smallest index it is (a triangle belongs to its first vertex's component);
 *   0 at every index that is no root.  Integer atomicAdd, one per wavefront where the wavefront shares a label.
 * pp_cc_keep_masks: root_keep [n_vertices] uint8 marks the roots of the components to keep -> vertex_keep [n_vertices] and
 *   triangle_keep [n_triangles] int32, 1 for a referenced vertex / a triangle of a marked component and 0 otherwise.
 * pp_cc_compact: vertex_scan / triangle_scan = the INCLUSIVE prefix sums of the two masks (the caller's scan).  Kept vertex v
 *   goes to row vertex_scan[v] - 1 of out_vertices [n_out_vertices,3] and out_index (= v); kept triangle i goes to row
 *   triangle_scan[i] - 1 of out_triangles with its three ids renumbered through vertex_scan: the kept rows stay in their
 *   relative order, the winding is untouched.  Rows from n_out_* on are not written.
 * A triangle with an index outside [0, n_vertices) is skipped by every kernel (the Python host refuses such a mesh first).
 * All refuse, before any GPU call: null pointers where rows exist, negative counts, more than 2^30 vertices or 2^29 triangles
 * (PP_ERR_UNSUPPORTED), a workspace that is too small. */
int pp_cc_workspace(int32_t n_vertices, int64_t* bytes);
int pp_cc_rounds(const int32_t* triangles, int32_t n_triangles, int32_t n_vertices, int32_t first_round, int32_t n_rounds,
                 int32_t* labels, void* work, int64_t work_bytes, int32_t* changed, void* stream);
int pp_cc_count(const int32_t* labels, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles, int32_t* vertex_counts,
                int32_t* triangle_counts, void* stream);
int pp_cc_keep_masks(const int32_t* labels, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                     const uint8_t* root_keep, int32_t* vertex_keep, int32_t* triangle_keep, void* stream);
int pp_cc_compact(const float* vertices, const int32_t* triangles, const int32_t* vertex_scan, const int32_t* triangle_scan,
                  int32_t n_vertices, int32_t n_triangles, float* out_vertices, int32_t* out_index, int32_t* out_triangles,
                  int32_t n_out_vertices, int32_t n_out_triangles, void* stream);

/* Signed distance of a triangle mesh at the nodes of a grid (csrc/pp_mesh_sdf.hip): the inverse of pp_mc_*.
 * vertices [V,3] fp32, triangles [T,3] int32.  A triangle with an index outside [0, V) takes part in nothing (the Python host
 * refuses such a mesh first).
 * Cell grid as for pp_dtu_*: origin (ox, oy, oz), cubic cells of `edge`, nx x ny x nz cells, a coordinate's cell is
 *   floor((p - o) / edge) in fp32 clamped into the grid, int64 keys (x ny + y) nz + z.  A triangle is registered in every cell
 *   its bounding box, padded by edge / 64 on every side, overlaps.  pp_msdf_bin_count writes counts [T] int64 (DEVICE), the
 *   caller scans them, pp_msdf_bin_emit writes the n_pairs (key, triangle) pairs triangle-major to keys / tris at offsets [T] =
 *   the exclusive scan; n_pairs above 2^31 - 1 is PP_ERR_UNSUPPORTED, nothing is truncated.  The caller sorts the pairs by key.
 * pp_msdf_nearest: the exact nearest point of the mesh for Q queries.  queries [Q,3], or NULL: the queries are the nodes
 *   (xs[i], ys[j], zs[k]) of the grid xs [X], ys [Y], zs [Z] in the order (i Y + j) Z + k, and Q must be X Y Z.  Per pair the
 *   closest point of the triangle is the best of the foot of the perpendicular (where it falls inside: barycentric weights from
 *   n . (ap x ac), n . (ab x ap), n = ab x ac, used only when n . n > 0) and the closest points of the three sides taken as
 *   segments (a side of no length is its end point), so a triangle without area takes part as a segment or a point.  fp32;
 *   d2 = (dx dx + dy dy) + dz dz between the query and the rounded closest point.  The winner is the smallest d2, ties to the
 *   lowest triangle index: a pure function of the inputs, whatever the cell grid.  Rings of cells at growing Chebyshev radius k
 *   around the query's cell; before ring k >= 2 the search ends if d2 <= ((k - 1.02) edge)^2 or (k - 1.02) edge >= max_dist
 *   (the margin covers the rounding of the cell coordinates, as for pp_dtu_nearest: at most 2^13 cells per axis).
 *   dist [Q] = sqrt(d2), closest [Q,3], tri [Q] int32; (inf, NaN, -1) where no triangle has d2 < max_dist^2 (max_dist = inf:
 *   no cap).  rings [Q] int32 (optional) receives the number of rings visited.
 * pp_msdf_crossings: counts [X+1,Y,Z] int32 (cleared by the call; pp_msdf_crossing_slots, a pure host function, gives its
 *   length).  For every column (j, k) the crossings of the line y = ys[j], z = zs[k] with the mesh are counted into the slot
 *   s = the number of nodes with xs[i] < x*, x* the crossing's abscissa: node i is inside iff the sum of the slots 0 .. i is
 *   odd (the caller's scan).  One wavefront per triangle walks the columns inside the triangle's (y, z) bounding box; integer
 *   atomicAdd only.  Coverage is decided in fp64 on the (y, z) projection by edge functions with the fill rule of the
 *   infinitesimal shift (+eps, +eps^2): a column on an edge belongs to the triangle iff the edge, walked with the interior on
 *   its positive side, has dz < 0, or dz = 0 and dy > 0.  Every edge function is evaluated from the lexicographically
 *   (y, z)-smaller end point and negated for the other direction, so the two triangles of an edge see the same number with
 *   opposite sign.  A triangle whose projection has no area contributes nothing.
 * xs, ys, zs must be strictly increasing (the caller's promise; X, Y, Z >= 1, X Y Z and (X + 1) Y Z at most 2^31 - 1).
 * No float atomics, no allocation, no host read; results are bit-reproducible.  All refuse, before any GPU call: null pointers
 * (except queries and rings), sizes below 1, a non-finite origin, a non-positive or non-finite edge, a max_dist that is NaN or
 * not positive. */
int pp_msdf_bin_count(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, float ox, float oy, float oz, float edge,
                      int32_t nx, int32_t ny, int32_t nz, int64_t* counts, void* stream);
int pp_msdf_bin_emit(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, float ox, float oy, float oz, float edge,
                     int32_t nx, int32_t ny, int32_t nz, const int64_t* offsets, int64_t* keys, int32_t* tris, int64_t n_pairs,
                     void* stream);
int pp_msdf_nearest(const float* queries, int32_t Q, const float* xs, const float* ys, const float* zs, int32_t X, int32_t Y, int32_t Z,
                    const float* vertices, int32_t V, const int32_t* triangles, int32_t T, const int64_t* keys, const int32_t* tris,
                    int32_t n_pairs, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz, float max_dist,
                    float* dist, float* closest, int32_t* tri, int32_t* rings, void* stream);
int pp_msdf_crossing_slots(int32_t X, int32_t Y, int32_t Z, int64_t* slots);
int pp_msdf_crossings(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, const float* xs, const float* ys,
                      const float* zs, int32_t X, int32_t Y, int32_t Z, int32_t* counts, void* stream);

/* ---------------------------------------------------------------- pose initialisation: PnP-RANSAC
 * lib/recon_scene.py:276-310 hands surface points and matched pixels to cv2.solvePnPRansac on the host; here they stay on the
 * device.  cv2's random draws and internal solver are not reproduced: the caller draws the samples, which makes the result a
 * pure, bit-reproducible function of its inputs.
 *   inputs: world [P,3], pix [P,2] (u = fx Xc / Zc + cx, v = fy Yc / Zc + cy, camera looking along +z: inverse_y), valid [P]
 *     uint8 (NULL = every row valid), intr [4] = (fx, fy, cx, cy) on the DEVICE, samples [H,4] int32, fallback [3,4];
 *   hypothesis h is VALID iff its four indices are in range, pairwise distinct and point at valid rows, and a P3P solve on the
 *     first three rows has a solution under which all four rows have positive depth (exactly collinear triples and zero side
 *     lengths have none); among those solutions the one with the smallest reprojection error at the fourth row is kept;
 *   score = rows with valid, depth > 0 and reprojection error < reproj_error (strict; compared as squares);
 *   winner = the largest score, ties to the lowest h; success needs score >= min_inliers;
 *   success: inliers [P] uint8 = the winner's mask (not recomputed after refinement), w2c [3,4] = its pose after refine_iters
 *     Gauss-Newton steps on the summed squared reprojection error of the inliers (left-multiplied SE(3) increment, 6 x 6
 *     normal equations by Cholesky; a non-positive pivot ends the refinement with the pose reached so far),
 *     info [2] int32 = (score, h);
 *   failure: w2c = fallback bit for bit, inliers all zero, info = (0, -1) - written by the kernel, no host decision.
 * fp32 in and out; the minimal solve, the scoring and the refinement run in fp64 with every sum in a fixed order.  Three
 * launches on `stream`, no atomics, no allocation, no host read.
 * Limits: 4 <= P <= 2^22, 1 <= H <= 2^16 (beyond the upper limits: PP_ERR_UNSUPPORTED), reproj_error > 0,
 * 0 <= refine_iters <= 1000, min_inliers >= 1.  pp_pnp_workspace (pure host function): bytes of `work`, 16-byte aligned, laid
 * out as poses double [H,12] at 0, validity flags int32 [H] at r(96 H), scores int32 [H] (-1 = invalid hypothesis) at
 * r(96 H) + r(4 H), with r(x) = x rounded up to a multiple of 256; all three are left behind for inspection.  Both entry points
 * refuse, before any GPU call: null pointers (except valid), sizes outside the limits, a workspace that is too small. */
int pp_pnp_workspace(int32_t P, int32_t H, int64_t* bytes);
int pp_pnp_ransac(const float* world, const float* pix, const uint8_t* valid, int32_t P, const float* intr, const int32_t* samples,
                  int32_t H, float reproj_error, int32_t refine_iters, int32_t min_inliers, const float* fallback, void* work,
                  int64_t work_bytes, float* w2c, uint8_t* inliers, int32_t* info, void* stream);

/* ---------------------------------------------------------------- mesh evaluation: DTU Chamfer distance
 * lib/dtu_eval.py::eval samples points from the triangles, thins them by radius and runs two nearest-neighbour passes on the
 * host; here the three stages run on device-resident points.  Sorting, scans and compaction are the caller's.
 * Sampling (lib/dtu_eval.py:70-89, decided in fp64 in the reference's operation order): vertices [V,3] fp64, triangles [T,3]
 *   int32.  v1 = p1 - p0, v2 = p2 - p0, l = sqrt((x x + y y) + z z), area2 = |v1 x v2|; a triangle with area2 > 0 has
 *   thr = thresh sqrt(l1 l2 / area2), n1 = floor(l1 / thr), n2 = floor(l2 / thr) and, when both are at least 1, the points
 *   (v1 a + v2 b) + p0 for 0 <= i <= n1, 0 <= j <= n2 with a = (i + 0.5) / n1, b = (j + 0.5) / n2, a + b < 1, i-major, rounded
 *   once to fp32.  pp_dtu_sample_count writes counts [T] int64 (DEVICE); a triangle with an index outside [0, V) counts 0, one
 *   whose n1 or n2 reaches 2^31 counts 2^31.  pp_dtu_sample_emit, given the same inputs and offsets [T] = the exclusive scan of
 *   counts, writes rows [0, n_points) of points [.,3] fp32 and nothing past them; n_points above 2^31 - 1 is PP_ERR_UNSUPPORTED.
 * Cell grid: origin (ox, oy, oz), cubic cells of `edge`, nx x ny x nz cells (each at most 2^20: PP_ERR_UNSUPPORTED beyond); a
 *   point's cell along an axis is floor((p - o) / edge) in fp32, clamped into the grid; pp_dtu_cell_keys writes the int64 keys
 *   (x ny + y) nz + z.  The two searches below take the points SORTED by key: points [N,3], keys [N], and order [N] int32 = the
 *   index each sorted point had before sorting.
 * Distance: d2 = (dx dx + dy dy) + dz dz in fp32.
 * pp_dtu_thin_rounds (lib/dtu_eval.py:98-106): the keep mask of walking the points in `order` order, a point still marked
 *   keeping itself and unmarking every point with d2 <= radius radius - computed in rounds on a state byte per sorted point
 *   (0 undecided, 1 kept, 2 removed): an undecided point is removed if a neighbour of lower order is kept, kept if every such
 *   neighbour is removed.  `work` (pp_dtu_thin_workspace: two state arrays of N bytes, each rounded up to 256) holds the
 *   state: round r reads the array at (r & 1) r256(N) and writes the other.  A call runs rounds first_round ..
 *   first_round + n_rounds - 1 (first_round = 0 clears the state first; 1 <= n_rounds <= 1024) and sets undecided[k]
 *   (DEVICE int32 [n_rounds]) to 1 iff a point is still undecided after its k-th round.  edge >= radius is required, and the
 *   caller leaves a margin for the rounding of the cell coordinate (poseprobe_amd/dtu_eval.py: 1 %, below 2^13 cells per axis).
 * pp_dtu_nearest (lib/dtu_eval.py:145-146, :158-159): d2 [Q] fp32 and idx [Q] int32 (in `order` numbering) of the exact nearest
 *   point of every query, ties to the lowest index; (inf, -1) where no point has d2 < max_dist max_dist.  The result does not
 *   depend on the grid (same margin rule as above).
 * All refuse, before any GPU call: null pointers, sizes below 1, a non-finite or non-positive thresh / edge / max_dist, a
 * negative radius, a workspace that is too small.  No allocation, no atomics, no host read. */
int pp_dtu_sample_count(const double* vertices, int32_t V, const int32_t* triangles, int32_t T, double thresh, int64_t* counts,
                        void* stream);
int pp_dtu_sample_emit(const double* vertices, int32_t V, const int32_t* triangles, int32_t T, double thresh, const int64_t* offsets,
                       float* points, int64_t n_points, void* stream);
int pp_dtu_cell_keys(const float* points, int32_t N, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz,
                     int64_t* keys, void* stream);
int pp_dtu_thin_workspace(int32_t N, int64_t* bytes);
int pp_dtu_thin_rounds(const float* points, const int64_t* keys, const int32_t* order, int32_t N, float ox, float oy, float oz,
                       float edge, int32_t nx, int32_t ny, int32_t nz, float radius, int32_t first_round, int32_t n_rounds, void* work,
                       int64_t work_bytes, int32_t* undecided, void* stream);
int pp_dtu_nearest(const float* queries, int32_t Q, const float* points, const int64_t* keys, const int32_t* order, int32_t P, float ox,
                   float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz, float max_dist, float* d2, int32_t* idx,
                   void* stream);

/* ---------------------------------------------------------------- image score: SSIM
 * lib/utils.py:792-838 (rgb_ssim) on device-resident image pairs: img0, img1 [V,H,W,C] fp32, contiguous, channels
 * last, 1 <= C <= 4.  The 1-D filter f_k = exp(-0.5 ((k - hw + shift) / filter_sigma)^2) / sum, hw = filter_size / 2 (integer),
 * shift = (2 hw - filter_size + 1) / 2, is computed on the host in fp64 and handed to the kernel by value (no upload, no copy in the stream).
 * Per channel the five images x, y, x x, y y, x y are blurred separably in `valid` mode, which leaves a map of
 * (H - filter_size + 1) x (W - filter_size + 1) x C values
 *   mu0 = B x, mu1 = B y, s00 = max(0, B xx - mu0^2), s11 = max(0, B yy - mu1^2), s01 = B xy - mu0 mu1 limited to
 *   sign(s01) min(sqrt(s00 s11), |s01|), c1 = (k1 max_val)^2, c2 = (k2 max_val)^2,
 *   ((2 mu0 mu1 + c1) (2 s01 + c2)) / ((mu0^2 + mu1^2 + c1) (s00 + s11 + c2)),
 * computed in fp64 from the fp32 inputs.  ssim [V] (DEVICE) receives the mean of each view's map; map (optional,
 * [V, H - fs + 1, W - fs + 1, C] fp32) the map, rounded once.  One work-group per tile of pp_ssim_tile x pp_ssim_tile map pixels
 * writes its fp64 sum to its own slot of `work` (pp_ssim_workspace, a pure host function: 8 bytes per tile and view, 8-byte
 * aligned) and a second kernel adds a view's slots in a fixed order: no atomics, no allocation, no host read, and a view's value
 * does not depend on the batch it is in, bit for bit.  Indexing is 64-bit; V times the tiles of a view must stay below 2^31
 * (PP_ERR_UNSUPPORTED beyond).  Both refuse, before any GPU call: null pointers (except map), V < 1, C outside 1..4, filter_size
 * outside 1..33, H or W below filter_size, a non-finite or non-positive filter_sigma / max_val, non-finite k1 / k2, a workspace
 * that is too small or misaligned. */
int pp_ssim_tile(int32_t* tile);
int pp_ssim_workspace(int32_t V, int32_t H, int32_t W, int32_t filter_size, int64_t* bytes);
int pp_ssim(const float* img0, const float* img1, int32_t V, int32_t H, int32_t W, int32_t C, int32_t filter_size,
            double filter_sigma, double max_val, double k1, double k2, void* work, int64_t work_bytes, float* ssim, float* map,
            void* stream);

/* ---------------------------------------------------------------- the two other branches of Voxurf.forward / Voxurf.inference
 * (csrc/pp_forward_variants.hip).
 * Plain-template geometry (use_deform=False, lib/voxurf_coarse.py:986-989, grad_mode 'interpolate' :458-467): no warp net.  With
 * G = softplus10(alpha) (sigmoid(softplus10(beta) sdf) - 0.5), sdf_final[M] is the trilinear sample of G at pts with
 * F.grid_sample semantics (align_corners=True, border padding: the coordinate is clipped to the grid) and gradient[M,3] the same
 * sample of the central differences (G[i+1] - G[i-1]) / 2 / voxel_size, a component being zero on the two boundary planes of its own
 * axis; alpha[M] is the NeuS alpha of pp_geometry_fwd.  Neither grid is materialised: 32 raw values per sample are mapped and
 * differenced in registers.  sdf_final may be NULL.  The grid needs two nodes along every axis. */
int pp_geometry_plain_fwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts, const float* viewdirs,
                          const int32_t* ray_id, const int32_t* count, int32_t capacity, float inv_s, float* alpha, float* gradient,
                          float* sdf_final, void* stream);
/* Upstream grads (any may be NULL): g_alpha[M], g_gradient[M,3], g_sdf_final[M].  Outputs: pts_grad[M,3] and viewdir_grad_s[M,3]
 * (accumulate=1: +=; a coordinate that the border padding clipped, u <= 0 or u >= size - 1, passes no gradient, as
 * F.grid_sample), sdf_ab_grad[2] (work-group sums, then one atomic += per value and work-group; caller zeroes; may be NULL). */
int pp_geometry_plain_bwd(const pp_scene* sc, const float* sdf_grid, const float* sdf_ab, const float* pts, const float* viewdirs,
                          const int32_t* ray_id, const int32_t* count, int32_t capacity, float inv_s, const float* g_alpha,
                          const float* g_gradient, const float* g_sdf_final, int32_t accumulate, float* pts_grad,
                          float* viewdir_grad_s, float* sdf_ab_grad, void* stream);
/* Weight-threshold compaction (fast_color_thres, lib/voxurf_coarse.py:996-1003, :1144-1151): of the samples
 * [ray_start[r], ray_start[r+1]) of every ray those with weights[i] > thres are kept, in order.  Outputs: kept_idx[j] = original
 * index of kept sample j, kept_ray_start[n_rays + 1] = the kept samples' exclusive prefix per ray, kept_count[1] = their number
 * (DEVICE), and the gathered rows pts_k[.,3], ray_id_k, step_k, alpha_k, gradient_k[.,3].  Every buffer holds `capacity` rows;
 * ray_start entries are read clamped to [0, capacity].  Rows past kept_count are left untouched.  Three launches (count, scan,
 * fill), one wavefront per ray, no atomics, no host read. */
int pp_keep_compact(const float* weights, const int32_t* ray_start, int32_t n_rays, int32_t capacity, float thres, const float* pts,
                    const int32_t* ray_id, const float* step, const float* alpha, const float* gradient, int32_t* kept_idx,
                    int32_t* kept_ray_start, int32_t* kept_count, float* pts_k, int32_t* ray_id_k, float* step_k, float* alpha_k,
                    float* gradient_k, void* stream);
/* Backward of the gather: every non-NULL full-length buffer (g_alpha[capacity], g_gradient / g_pts / g_view [capacity,3]) is zeroed
 * and row kept_idx[j] then receives row j of its kept twin, j < kept_count (one-to-one: plain stores, no atomics). */
int pp_keep_scatter_bwd(const int32_t* kept_idx, const int32_t* kept_count, int32_t capacity, const float* g_alpha_k,
                        const float* g_gradient_k, const float* g_pts_k, const float* g_view_k, float* g_alpha, float* g_gradient,
                        float* g_pts, float* g_view, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSEPROBE_HIP_H */
