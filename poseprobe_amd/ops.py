"""Thin, allocation-explicit Python wrappers over the C ABI (include/poseprobe_hip.h).

One function per entry point; tensors are torch CUDA tensors used purely as device buffers (torch is
plumbing: memory + streams).  Error behaviour mirrors the reference extension
(lib/cuda/render_utils.cpp:46-48 CHECK_INPUT): non-CUDA or non-contiguous inputs raise RuntimeError.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import pp_scene


def _ptr(t, dtype=None, name='tensor'):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f'{name} must be {dtype}, got {t.dtype}')
    return ctypes.c_void_p(t.data_ptr())


def _f(t, name='tensor'):
    return _ptr(t, torch.float32, name)


def _i(t, name='tensor'):
    return _ptr(t, torch.int32, name)


def _u8(t, name='tensor'):
    return _ptr(t, torch.uint8, name)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_scene(xyz_min, xyz_max, world_size, voxel_size, stepsize, near, far, bg, out_range=1.0, k0_dim=12,
               pos_pe=5, view_pe=1, sdf_index_exact=None):
    sc = pp_scene()
    for i in range(3):
        sc.xyz_min[i] = float(xyz_min[i])
        sc.xyz_max[i] = float(xyz_max[i])
        sc.size[i] = int(world_size[i])
    sc.voxel_size = float(np.float32(voxel_size))
    sc.stepsize = float(stepsize)
    sc.near_clip = float(near)
    sc.far_clip = float(far)
    sc.bg = float(bg)
    # voxurf_coarse.py:700
    sc.n_samples = int(np.linalg.norm(np.array([int(w) for w in world_size]) + 1) / stepsize) + 1
    sc.out_range = float(out_range)
    sc.k0_dim, sc.pos_pe, sc.view_pe = int(k0_dim), int(pos_pe), int(view_pe)
    if sdf_index_exact is None:         # host-side switch (PP_SDF_INDEX_EXACT=1): the mathematically intended voxel index above 2^24 voxels
        import os
        sdf_index_exact = os.environ.get('PP_SDF_INDEX_EXACT') == '1'
    sc.sdf_index_exact = int(bool(sdf_index_exact))
    return sc


RGBNET_PARAMS = 128 * 64 + 128 + 2 * (128 * 128 + 128) + 3 * 128 + 3
WARP_PARAMS = 128 * 3 + 128 + 3 * (128 * 128 + 128) + 4 * 128 + 4
FEAT_LD = 64


# ------------------------------------------------------------------------------------------- pose / rays
def pose_fwd(se3, w2c_init, refine_mask, w2c, c2w, jac):
    V = se3.shape[0]
    _lib.call('pp_pose_fwd', _f(se3), _f(w2c_init), _i(refine_mask), V, _f(w2c), _f(c2w), _f(jac), _stream())


def step_begin(se3, w2c_init, refine_mask, w2c, c2w, jac, scalars, step_dev, zero_block, warp_params=None, rgbnet_params=None,
               pack=None, ctx=None):
    """Head of a train step in one launch (pp_step_begin): pose_fwd; step_dev[:len(scalars)] = scalars (a host sequence of at most
    32 floats, handed to the kernel by value: no copy in the stream); zero_block = 0; with `pack`, mlp_pack of the two parameter
    blocks, recorded in `ctx` as mlp_pack records it."""
    vals = np.ascontiguousarray(scalars, dtype=np.float32)
    n = vals.shape[0]
    host = (ctypes.c_float * max(n, 1)).from_buffer_copy(vals.tobytes() if n else bytes(4))
    _lib.call('pp_step_begin', _f(se3), _f(w2c_init), _i(refine_mask), se3.shape[0], _f(w2c), _f(c2w), _f(jac),
              ctypes.cast(host, ctypes.c_void_p), n, _f(step_dev), _f(zero_block), 0 if zero_block is None else zero_block.numel(),
              _f(warp_params), _f(rgbnet_params), _f(pack), _h(ctx), _stream())


def pose_bwd(jac, c2w_grad, se3_grad):
    _lib.call('pp_pose_bwd', _f(jac), _f(c2w_grad), se3_grad.shape[0], _f(se3_grad), _stream())


def raygen_select_fwd(sc, ray_idx, c2w, intr, H, W, inverse_y, normalize, images, masks, rays_o, rays_d, viewdirs,
                      target, mask_px):
    _lib.call('pp_raygen_select_fwd', ctypes.byref(sc), _i(ray_idx), ray_idx.shape[0], _f(c2w), _f(intr),
              c2w.shape[0], H, W, int(inverse_y), int(normalize), _f(images), _f(masks), _f(rays_o), _f(rays_d),
              _f(viewdirs), _f(target), _f(mask_px), _stream())


def raygen_select_bwd(sc, ray_idx, c2w, intr, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step,
                      vgrad_s, g_o, g_d, g_v, g_depth, g_o_out, g_d_out, g_v_out, c2w_grad):
    n_views = c2w.shape[0] if c2w is not None else 0
    _lib.call('pp_raygen_select_bwd', ctypes.byref(sc), _i(ray_idx), rays_o.shape[0], _f(c2w), _f(intr), n_views,
              H, W, int(inverse_y), _f(rays_o), _f(rays_d), _f(t_min), _i(ray_start), _f(pts_grad), _f(step),
              _f(vgrad_s), _f(g_o), _f(g_d), _f(g_v), _f(g_depth), _f(g_o_out), _f(g_d_out), _f(g_v_out),
              _f(c2w_grad), _stream())


def sample_dense(sc, rays_o, rays_d, jitter, capacity, t_min, t_max, ray_start, count, pts, ray_id, step_k, step,
                 mask_keep=None):
    _lib.call('pp_sample_dense', ctypes.byref(sc), _f(rays_o), _f(rays_d), _f(jitter), rays_o.shape[0], capacity,
              _f(t_min), _f(t_max), _i(ray_start), _i(count), _f(pts), _i(ray_id), _i(step_k), _f(step),
              _ptr(mask_keep, torch.uint8), _stream())


def sample_var(sc, rays_o, rays_d, capacity, t_min, t_max, n_steps, ray_start, count, pts, ray_id, step_id):
    _lib.call('pp_sample_var', ctypes.byref(sc), _f(rays_o), _f(rays_d), rays_o.shape[0], capacity, _f(t_min),
              _f(t_max), _i(n_steps), _i(ray_start), _i(count), _f(pts), _i(ray_id), _i(step_id), _stream())


# ------------------------------------------------------------------------------------------- scan / composite
def alpha2weight_fwd(alpha, ray_start, n_rays, weights, T, alphainv_last, i_end):
    _lib.call('pp_alpha2weight_fwd', _f(alpha), _i(ray_start), n_rays, _f(weights), _f(T), _f(alphainv_last),
              _i(i_end), _stream())


def alpha2weight_bwd(alpha, weights, T, alphainv_last, ray_start, i_end, n_rays, grad_weights, grad_last, grad_alpha):
    _lib.call('pp_alpha2weight_bwd', _f(alpha), _f(weights), _f(T), _f(alphainv_last), _i(ray_start), _i(i_end),
              n_rays, _f(grad_weights), _f(grad_last), _f(grad_alpha), _stream())


def march_fwd(alpha, rgb, step_w, nrm_in, ray_start, n_rays, bg, weights, T, alphainv_last, i_end, rgb_marched,
              rgb_pre, cum_weights, depth_acc, normal_marched):
    _lib.call('pp_march_fwd', _f(alpha), _f(rgb), _f(step_w), _f(nrm_in), _i(ray_start), n_rays, float(bg),
              _f(weights), _f(T), _f(alphainv_last), _i(i_end), _f(rgb_marched), _f(rgb_pre), _f(cum_weights),
              _f(depth_acc), _f(normal_marched), _stream())


def march_bwd(alpha, rgb, step_w, weights, T, alphainv_last, ray_start, i_end, n_rays, bg, rgb_pre, g_rgbm, g_cw,
              g_last, g_depth, g_weights, grad_alpha, grad_rgb):
    _lib.call('pp_march_bwd', _f(alpha), _f(rgb), _f(step_w), _f(weights), _f(T), _f(alphainv_last), _i(ray_start),
              _i(i_end), n_rays, float(bg), _f(rgb_pre), _f(g_rgbm), _f(g_cw), _f(g_last), _f(g_depth),
              _f(g_weights), _f(grad_alpha), _f(grad_rgb), _stream())


MARCH_LOSS_MAX_SAMPLES = 192       # samples of one ray that march_loss_bwd's kernel holds (pp_march_loss_workspace refuses more)
STEP_SCALARS_MAX = 32              # floats that step_begin hands to its kernel by value


def march_loss_workspace(n_rays, sample_cap):
    """Bytes of the workspace of march_loss_bwd (zero before the first call); raises PoseProbeError when the kernel cannot hold
    `sample_cap` samples of a ray - the caller then takes march_fwd / loss_rays / march_bwd."""
    b = ctypes.c_int64()
    _lib.call('pp_march_loss_workspace', int(n_rays), int(sample_cap), ctypes.byref(b))
    return b.value


def march_loss_bwd(alpha, rgb, step_w, ray_start, n_rays, sample_cap, bg, weights, T, alphainv_last, i_end, rgb_marched, rgb_pre,
                   cum_weights, depth_acc, target, mask_px, mask_sum, w_main, w_entropy, w_mask, loss_scale, g_rgbm, g_last, g_cw,
                   loss_out, g_depth, g_weights, grad_alpha, grad_rgb, work):
    """march_fwd -> loss_rays -> march_bwd of every ray by one wavefront, in one launch (pp_march_loss_bwd)."""
    _lib.call('pp_march_loss_bwd', _f(alpha), _f(rgb), _f(step_w), _i(ray_start), n_rays, int(sample_cap), float(bg), _f(weights),
              _f(T), _f(alphainv_last), _i(i_end), _f(rgb_marched), _f(rgb_pre), _f(cum_weights), _f(depth_acc), _f(target),
              _f(mask_px), _f(mask_sum), float(w_main), float(w_entropy), float(w_mask), float(loss_scale), _f(g_rgbm), _f(g_last),
              _f(g_cw), _f(loss_out), _f(g_depth), _f(g_weights), _f(grad_alpha), _f(grad_rgb), _u8(work), work.numel(), _stream())


# ------------------------------------------------------------------------------------------- geometry / colour
def geometry_fwd(sc, sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient,
                 sdf_final, sdf_deform, grad_deform):
    _lib.call('pp_geometry_fwd', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(warp_out), _f(viewdirs),
              _i(ray_id), _i(count), capacity, float(inv_s), _f(alpha), _f(gradient), _f(sdf_final), _f(sdf_deform),
              _f(grad_deform), _stream())


def geometry_bwd(sc, sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                 g_sdf_final, g_sdf_deform, g_grad_deform, g_correction, accumulate, warp_out_grad, pts_grad, vgrad_s,
                 sdf_ab_grad):
    _lib.call('pp_geometry_bwd', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(warp_out), _f(viewdirs),
              _i(ray_id), _i(count), capacity, float(inv_s), _f(g_alpha), _f(g_gradient), _f(g_sdf_final),
              _f(g_sdf_deform), _f(g_grad_deform), _f(g_correction), int(accumulate), _f(warp_out_grad),
              _f(pts_grad), _f(vgrad_s), _f(sdf_ab_grad), _stream())


def color_feat_fwd(sc, k0_cl, pts, viewdirs, ray_id, gradient, pe_w, count, capacity, feat):
    _lib.call('pp_color_feat_fwd', ctypes.byref(sc), _f(k0_cl), _f(pts), _f(viewdirs), _i(ray_id), _f(gradient),
              _f(pe_w), _i(count), capacity, _f(feat), _stream())


def color_feat_bwd(sc, k0_cl, pts, viewdirs, ray_id, gradient, pe_w, count, capacity, feat_grad, k0_grad_cl, pts_grad,
                   gradient_grad, vgrad_s):
    _lib.call('pp_color_feat_bwd', ctypes.byref(sc), _f(k0_cl), _f(pts), _f(viewdirs), _i(ray_id), _f(gradient),
              _f(pe_w), _i(count), capacity, _f(feat_grad), _f(k0_grad_cl), _f(pts_grad), _f(gradient_grad),
              _f(vgrad_s), _stream())


def geometry_bwd_priors(sc, sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                        w_eikonal, w_deform, loss_scale, accumulate, warp_out_grad, pts_grad, vgrad_s, sdf_ab_grad, loss_out,
                        batch_norm=None):
    _lib.call('pp_geometry_bwd_priors', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(warp_out), _f(viewdirs),
              _i(ray_id), _i(count), capacity, float(inv_s), _f(g_alpha), _f(g_gradient), float(w_eikonal), float(w_deform),
              float(loss_scale), int(accumulate), _f(warp_out_grad), _f(pts_grad), _f(vgrad_s), _f(sdf_ab_grad),
              _f(loss_out), _f(batch_norm), _stream())


def geometry_color_feat_fwd(sc, sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient,
                           sdf_final, sdf_deform, grad_deform, k0_cl, pe_w, feat):
    """geometry_fwd and color_feat_fwd as two roles of one launch (k0_dim = 12, pos_pe = 5, view_pe = 1 only)."""
    _lib.call('pp_geometry_color_feat_fwd', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(warp_out), _f(viewdirs),
              _i(ray_id), _i(count), capacity, float(inv_s), _f(alpha), _f(gradient), _f(sdf_final), _f(sdf_deform),
              _f(grad_deform), _f(k0_cl), _f(pe_w), _f(feat), _stream())


# ------------------------------------------------------------------------------------------- forward variants
def geometry_plain_fwd(sc, sdf_grid, sdf_ab, pts, viewdirs, ray_id, count, capacity, inv_s, alpha, gradient, sdf_final=None):
    """Geometry of Voxurf.forward(use_deform=False): grid_sample lookups of the mapped template and of its central differences."""
    _lib.call('pp_geometry_plain_fwd', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(viewdirs), _i(ray_id), _i(count),
              capacity, float(inv_s), _f(alpha), _f(gradient), _f(sdf_final), _stream())


def geometry_plain_bwd(sc, sdf_grid, sdf_ab, pts, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient, g_sdf_final,
                       accumulate, pts_grad, vgrad_s, sdf_ab_grad):
    _lib.call('pp_geometry_plain_bwd', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(viewdirs), _i(ray_id), _i(count),
              capacity, float(inv_s), _f(g_alpha), _f(g_gradient), _f(g_sdf_final), int(accumulate), _f(pts_grad), _f(vgrad_s),
              _f(sdf_ab_grad), _stream())


def keep_compact(weights, ray_start, n_rays, capacity, thres, pts, ray_id, step, alpha, gradient, kept_idx, kept_ray_start,
                 kept_count, pts_k, ray_id_k, step_k, alpha_k, gradient_k):
    """The samples with weights > thres of every ray, in order: indices, new ray_start, device-side count, gathered rows."""
    _lib.call('pp_keep_compact', _f(weights), _i(ray_start), int(n_rays), int(capacity), float(thres), _f(pts), _i(ray_id), _f(step),
              _f(alpha), _f(gradient), _i(kept_idx), _i(kept_ray_start), _i(kept_count), _f(pts_k), _i(ray_id_k), _f(step_k),
              _f(alpha_k), _f(gradient_k), _stream())


def keep_scatter_bwd(kept_idx, kept_count, capacity, g_alpha_k, g_gradient_k, g_pts_k, g_view_k, g_alpha, g_gradient, g_pts, g_view):
    """Rows of the kept gradients back to their original rows, exact zeros everywhere else."""
    _lib.call('pp_keep_scatter_bwd', _i(kept_idx), _i(kept_count), int(capacity), _f(g_alpha_k), _f(g_gradient_k), _f(g_pts_k),
              _f(g_view_k), _f(g_alpha), _f(g_gradient), _f(g_pts), _f(g_view), _stream())


# ------------------------------------------------------------------------------------------- ordered gradient flushes
def ordered_workspace(work_groups, capacity, n_rays):
    """Bytes of the ordered-flush workspace (pp_ordered_workspace): work_groups = the largest persistent grid the MLP kernels
    will use (the device's compute-unit count, or option mlp_wgs when set)."""
    b = ctypes.c_int64()
    _lib.call('pp_ordered_workspace', int(work_groups), int(capacity), int(n_rays), ctypes.byref(b))
    return b.value


def ordered_attach(ctx, work, work_groups, capacity, n_rays):
    """Record `work` (uint8 tensor of ordered_workspace(...) bytes; None = detach) in `ctx` (an _lib.Context, required): the MLP
    backward calls handed this context, geometry_bwd_priors_ordered and raygen_select_bwd_ordered then add the parameter
    gradients up in a fixed order instead of by float atomics.  The caller keeps `work` alive while such calls are in flight."""
    if ctx is None:
        raise ValueError('ordered_attach needs a context of its own (the default context is shared by everybody)')
    _lib.call('pp_ordered_attach', ctx.handle, _u8(work), 0 if work is None else int(work.numel()), int(work_groups),
              int(capacity), int(n_rays))


def geometry_bwd_priors_ordered(sc, sdf_grid, sdf_ab, pts, warp_out, viewdirs, ray_id, count, capacity, inv_s, g_alpha, g_gradient,
                                w_eikonal, w_deform, loss_scale, accumulate, warp_out_grad, pts_grad, vgrad_s, sdf_ab_grad, loss_out,
                                batch_norm, ctx):
    _lib.call('pp_geometry_bwd_priors_ordered', ctypes.byref(sc), _f(sdf_grid), _f(sdf_ab), _f(pts), _f(warp_out), _f(viewdirs),
              _i(ray_id), _i(count), capacity, float(inv_s), _f(g_alpha), _f(g_gradient), float(w_eikonal), float(w_deform),
              float(loss_scale), int(accumulate), _f(warp_out_grad), _f(pts_grad), _f(vgrad_s), _f(sdf_ab_grad),
              _f(loss_out), _f(batch_norm), ctx.handle, _stream())


def raygen_select_bwd_ordered(sc, ray_idx, c2w, intr, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step,
                              vgrad_s, g_o, g_d, g_v, g_depth, g_o_out, g_d_out, g_v_out, c2w_grad, ctx):
    _lib.call('pp_raygen_select_bwd_ordered', ctypes.byref(sc), _i(ray_idx), rays_o.shape[0], _f(c2w), _f(intr), c2w.shape[0],
              H, W, int(inverse_y), _f(rays_o), _f(rays_d), _f(t_min), _i(ray_start), _f(pts_grad), _f(step),
              _f(vgrad_s), _f(g_o), _f(g_d), _f(g_v), _f(g_depth), _f(g_o_out), _f(g_d_out), _f(g_v_out),
              _f(c2w_grad), ctx.handle, _stream())


def k0_pack_samples(pts, feat_grad, count, capacity, k0_dim, packed):
    _lib.call('pp_k0_pack_samples', _f(pts), _f(feat_grad), _i(count), capacity, int(k0_dim), _f(packed), _stream())


def k0_scatter_packed(sc, packed, n_shards, capacity, k0_grad_cl, touched=None):
    _lib.call('pp_k0_scatter_packed', ctypes.byref(sc), _f(packed), int(n_shards), capacity, _f(k0_grad_cl), _u8(touched),
              _stream())


def k0_scatter_samples(sc, pts, count, capacity, feat_grad, k0_grad_cl, touched=None):
    _lib.call('pp_k0_scatter_samples', ctypes.byref(sc), _f(pts), _i(count), capacity, _f(feat_grad), _f(k0_grad_cl),
              _u8(touched), _stream())


def k0_scatter_sorted_workspace(n_samples):
    """Bytes of device workspace the deterministic scatters need for n_samples = n_shards * capacity samples."""
    b = ctypes.c_int64()
    _lib.call('pp_k0_scatter_sorted_workspace', int(n_samples), ctypes.byref(b))
    return b.value


def k0_scatter_samples_sorted(sc, pts, count, capacity, feat_grad, k0_grad_cl, work, touched=None):
    """Deterministic pp_k0_scatter_samples: contributions sorted by voxel and added in sample order (work: uint8 tensor)."""
    _lib.call('pp_k0_scatter_samples_sorted', ctypes.byref(sc), _f(pts), _i(count), capacity, _f(feat_grad), _f(k0_grad_cl),
              _u8(touched), _u8(work), int(work.numel()), _stream())


def k0_scatter_packed_sorted(sc, packed, n_shards, capacity, k0_grad_cl, work, touched=None):
    _lib.call('pp_k0_scatter_packed_sorted', ctypes.byref(sc), _f(packed), int(n_shards), capacity, _f(k0_grad_cl), _u8(touched),
              _u8(work), int(work.numel()), _stream())


# ------------------------------------------------------------------------------------------- MLPs
# Every wrapper of an option-dependent entry point takes `ctx`: an _lib.Context, or None = the host's default context.
Context = _lib.Context
_h = _lib.handle


def mlp_pack_workspace():
    """Floats of the weight-pack buffer of pp_mlp_pack."""
    n = ctypes.c_int64()
    _lib.call('pp_mlp_pack_workspace', ctypes.byref(n))
    return n.value


def mlp_pack(warp_params, rgbnet_params, pack, ctx=None):
    """Pack both nets' weights for the split-precision MLP kernels and record the pack in `ctx` for exactly these two parameter
    tensors; must be repeated (or mlp_pack_invalidate called) whenever their values change."""
    _lib.call('pp_mlp_pack', _f(warp_params), _f(rgbnet_params), _f(pack), _h(ctx), _stream())


def mlp_pack_invalidate(ctx=None):
    _lib.call('pp_mlp_pack_invalidate', _h(ctx))


def warp_lean_begin(acts, scratch, params, ctx=None):
    """Open a lean scope of the warp net for these buffers (pp_warp_lean_begin): until warp_lean_end, warp_fwd / warp_bwd /
    warp_bwd_data / warp_bwd_weights called with `ctx` and exactly these tensors leave out the tangent rows of X0 and Ybar3,
    which the weight-gradient kernel rebuilds.  Records nothing with option warp_lean = 0 or without the split-precision kernels."""
    _lib.call('pp_warp_lean_begin', _f(acts), _f(scratch), _f(params), _h(ctx))


def warp_lean_end(ctx=None):
    _lib.call('pp_warp_lean_end', _h(ctx))


def wgrad_join_begin(ctx=None):
    """Open a join scope of the weight gradients (pp_wgrad_join_begin): until wgrad_join_end, rgbnet_bwd called with `ctx` leaves
    its weight-gradient chain as a record in the context, and the next warp_bwd / warp_bwd_weights with `ctx`, the same `count`
    tensor and the same stream carries it in its own launch; whatever cannot be joined is launched as outside the scope."""
    _lib.call('pp_wgrad_join_begin', _h(ctx))


def wgrad_join_end(ctx=None, launch_pending=True):
    """Close the scope; a record nobody took is launched on its own, or dropped with launch_pending=False (the pass raised)."""
    _lib.call('pp_wgrad_join_end', _h(ctx), int(bool(launch_pending)))


def rgbnet_fwd(params, feat, count, capacity, acts, rgb, ctx=None):
    _lib.call('pp_rgbnet_fwd', _f(params), _f(feat), _i(count), capacity, _f(acts), _f(rgb), _h(ctx), _stream())


def rgbnet_bwd(params, feat, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, ctx=None):
    _lib.call('pp_rgbnet_bwd', _f(params), _f(feat), _f(acts), _f(rgb), _f(rgb_grad), _i(count), capacity,
              _f(scratch), _f(params_grad), _f(feat_grad), _h(ctx), _stream())


def warp_fwd(params, pts, count, capacity, out_range, acts, out, ctx=None):
    _lib.call('pp_warp_fwd', _f(params), _f(pts), _i(count), capacity, float(out_range), _f(acts), _f(out), _h(ctx), _stream())


def warp_bwd(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, ctx=None):
    _lib.call('pp_warp_bwd', _f(params), _f(pts), _f(acts), _f(out_grad), _i(count), capacity, float(out_range),
              _f(scratch), _f(params_grad), _f(pts_grad), _h(ctx), _stream())


def mlp_workspaces(capacity):
    """-> {'rgbnet': (acts, scratch), 'warp': (acts, scratch)} in floats, from the library's workspace queries."""
    out = {}
    for name in ('rgbnet', 'warp'):
        a, s = ctypes.c_int64(), ctypes.c_int64()
        _lib.call(f'pp_{name}_workspace', int(capacity), ctypes.byref(a), ctypes.byref(s))
        out[name] = (a.value, s.value)
    return out


def warp_bwd_data(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, ctx=None):
    """-> stage2: the value to hand to warp_bwd_weights (which stage owns the hidden layers' bias gradients)."""
    stage2 = ctypes.c_int32()
    _lib.call('pp_warp_bwd_data', _f(params), _f(pts), _f(acts), _f(out_grad), _i(count), capacity, float(out_range),
              _f(scratch), _f(params_grad), _f(pts_grad), ctypes.byref(stage2), _h(ctx), _stream())
    return stage2.value


def warp_bwd_weights(acts, scratch, count, capacity, params_grad, stage2, ctx=None):
    _lib.call('pp_warp_bwd_weights', _f(acts), _f(scratch), _i(count), capacity, _f(params_grad), int(stage2), _h(ctx), _stream())


def rgbnet_bwd_data(params, acts, rgb, rgb_grad, count, capacity, scratch, params_grad, feat_grad, ctx=None):
    stage2 = ctypes.c_int32()
    _lib.call('pp_rgbnet_bwd_data', _f(params), _f(acts), _f(rgb), _f(rgb_grad), _i(count), capacity, _f(scratch),
              _f(params_grad), _f(feat_grad), ctypes.byref(stage2), _h(ctx), _stream())
    return stage2.value


def rgbnet_bwd_weights(feat, acts, scratch, count, capacity, params_grad, stage2, ctx=None):
    _lib.call('pp_rgbnet_bwd_weights', _f(feat), _f(acts), _f(scratch), _i(count), capacity, _f(params_grad), int(stage2),
              _h(ctx), _stream())


# ------------------------------------------------------------------------------------------- losses / optimiser
def loss_rays(rgb_marched, alphainv_last, cum_weights, target, mask_px, mask_sum, w_main, w_entropy, w_mask,
              loss_scale, g_rgbm, g_last, g_cw, loss_out, batch_norm=None, march=None):
    """march: (alpha, rgb, step_w, ray_start, sample_cap, bg, weights, T, i_end, rgb_pre, depth_acc, grad_alpha, grad_rgb, work) - the
    rays have not been composited yet: march_fwd before the losses and march_bwd behind them run in the same launch, a wavefront
    per ray (march_loss_bwd); rgb_marched / alphainv_last / cum_weights are then outputs as well.  Not with batch_norm."""
    if march is not None:
        if batch_norm is not None:
            raise ValueError('loss_rays(march=...) has no batch_norm: composite and differentiate with the separate calls')
        alpha, rgb, step_w, ray_start, sample_cap, bg, weights, T, i_end, rgb_pre, depth_acc, grad_alpha, grad_rgb, work = march
        march_loss_bwd(alpha, rgb, step_w, ray_start, rgb_marched.shape[0], sample_cap, bg, weights, T, alphainv_last, i_end,
                       rgb_marched, rgb_pre, cum_weights, depth_acc, target, mask_px, mask_sum, w_main, w_entropy, w_mask,
                       loss_scale, g_rgbm, g_last, g_cw, loss_out, None, None, grad_alpha, grad_rgb, work)
        return
    _lib.call('pp_loss_rays', _f(rgb_marched), _f(alphainv_last), _f(cum_weights), _f(target), _f(mask_px),
              _f(mask_sum), rgb_marched.shape[0], float(w_main), float(w_entropy), float(w_mask), float(loss_scale),
              _f(g_rgbm), _f(g_last), _f(g_cw), _f(loss_out), _f(batch_norm), _stream())


def loss_samples(gradient, grad_deform, warp_out, sdf_deform, count, capacity, w_eik, w_deform, loss_scale, g_gradient,
                 g_grad_deform, g_correction, g_sdf_deform, loss_out, batch_norm=None):
    _lib.call('pp_loss_samples', _f(gradient), _f(grad_deform), _f(warp_out), _f(sdf_deform), _i(count), capacity,
              float(w_eik), float(w_deform), float(loss_scale), _f(g_gradient), _f(g_grad_deform), _f(g_correction),
              _f(g_sdf_deform), _f(loss_out), _f(batch_norm), _stream())


def _tail_args(tail):
    """Arguments of pp_grid_tv_adam_step_tail after the grid pass's own ones.  tail: dict(
    flat=(p, grad, m, v, seg_end, seg_lr, beta1, beta2, eps)            Adam over the flat block (grad zeroed),
    pose=(se3, grad, m, v, lr[1], beta1, beta2, eps, update) or None    Adam over the se3 block when `update`,
    rays=(sc, ray_idx, c2w, intr, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step, vgrad_s, jac, c2w_grad,
          arrive) or None                                               ray + pose backward ahead of it (needs pose; c2w_grad and
                                                                        arrive [1] int32 are zero on entry and on exit))."""
    fp, fg, fm, fv, seg_end, seg_lr, b1, b2, eps = tail['flat']
    out = [_f(fp), _f(fg), _f(fm), _f(fv), fp.numel(), _i(seg_end), _f(seg_lr), seg_end.numel(), float(b1), float(b2), float(eps)]
    pose, rays = tail.get('pose'), tail.get('rays')
    if pose is None:
        out += [None, None, None, None, 0, None, 0., 0., 0., 0]
    else:
        se3, g, m, v, lr, b1, b2, eps, update = pose
        out += [_f(se3), _f(g), _f(m), _f(v), se3.numel() // 6, _f(lr), float(b1), float(b2), float(eps), int(bool(update))]
    if rays is None:
        out += [None, None, 0, None, None, 0, 0, 0] + [None] * 10
    else:
        sc, ray_idx, c2w, intr, H, W, inverse_y, rays_o, rays_d, t_min, ray_start, pts_grad, step, vgrad_s, jac, c2w_grad, arrive = rays
        out += [ctypes.byref(sc), _i(ray_idx), rays_o.shape[0], _f(c2w), _f(intr), H, W, int(inverse_y), _f(rays_o), _f(rays_d),
                _f(t_min), _i(ray_start), _f(pts_grad), _f(step), _f(vgrad_s), _f(jac), _f(c2w_grad), _i(arrive)]
    return out


def grid_tv_adam_step(p_in, p_out, grad, exp_avg, exp_avg_sq, size, channels, x_begin, x_end, tv_scale, grad_scale, lr,
                      beta1, beta2, eps, step, tv_out, ctx=None, tail=None):
    """tail (see _tail_args): the launch also carries the end of the step (pp_grid_tv_adam_step_tail)."""
    if tail is not None:            # the dense pass of the tail-carrying entry point: no touched-voxel maps
        _lib.call('pp_grid_tv_adam_step_tail', _f(p_in), _f(p_out), _f(grad), _f(exp_avg), _f(exp_avg_sq),
                  int(size[0]), int(size[1]), int(size[2]), channels, x_begin, x_end, float(tv_scale), float(grad_scale),
                  float(lr), float(beta1), float(beta2), float(eps), int(step), _f(tv_out), None, None, *_tail_args(tail),
                  _h(ctx), _stream())
        return
    _lib.call('pp_grid_tv_adam_step', _f(p_in), _f(p_out), _f(grad), _f(exp_avg), _f(exp_avg_sq),
              int(size[0]), int(size[1]), int(size[2]), channels, x_begin, x_end, float(tv_scale), float(grad_scale),
              float(lr), float(beta1), float(beta2), float(eps), int(step), _f(tv_out), _h(ctx), _stream())


def grid_tv_adam_step_sparse(p_in, p_out, grad, exp_avg, exp_avg_sq, size, channels, x_begin, x_end, tv_scale, grad_scale,
                             lr, beta1, beta2, eps, step, tv_out, touched, touched_clear, ctx=None, tail=None):
    """tail (see _tail_args): the launch also carries the end of the step (pp_grid_tv_adam_step_tail)."""
    grid = (_f(p_in), _f(p_out), _f(grad), _f(exp_avg), _f(exp_avg_sq),
            int(size[0]), int(size[1]), int(size[2]), channels, x_begin, x_end, float(tv_scale), float(grad_scale),
            float(lr), float(beta1), float(beta2), float(eps), int(step), _f(tv_out), _u8(touched), _u8(touched_clear))
    if tail is None:
        _lib.call('pp_grid_tv_adam_step_sparse', *grid, _h(ctx), _stream())
    else:
        _lib.call('pp_grid_tv_adam_step_tail', *grid, *_tail_args(tail), _h(ctx), _stream())


def grid_tv_value(p, size, channels, out):
    _lib.call('pp_grid_tv_value', _f(p), int(size[0]), int(size[1]), int(size[2]), channels, _f(out), _stream())


def adam_flat(p, grad, exp_avg, exp_avg_sq, seg_end, seg_lr, grad_scale, beta1, beta2, eps, step, zero_grad):
    _lib.call('pp_adam_flat', _f(p), _f(grad), _f(exp_avg), _f(exp_avg_sq), p.numel(), _i(seg_end), _f(seg_lr),
              seg_end.numel(), float(grad_scale), float(beta1), float(beta2), float(eps), int(step), int(zero_grad),
              _stream())


def grid_sample_fwd(sc, grid_cl, channels, pts, border, out):
    _lib.call('pp_grid_sample_fwd', ctypes.byref(sc), _f(grid_cl), channels, _f(pts), pts.shape[0], int(border), _f(out),
              _stream())


def grid_sample_bwd(sc, grid_cl, channels, pts, border, out_grad, grid_grad_cl, pts_grad):
    _lib.call('pp_grid_sample_bwd', ctypes.byref(sc), _f(grid_cl), channels, _f(pts), pts.shape[0], int(border),
              _f(out_grad), _f(grid_grad_cl), _f(pts_grad), _stream())


def grid_tv_grad(p, size, channels, scale, g_scalar, grad):
    _lib.call('pp_grid_tv_grad', _f(p), int(size[0]), int(size[1]), int(size[2]), channels, float(scale), _f(g_scalar),
              _f(grad), _stream())


def sdf_first_crossing(sdf, ray_start, step_k, n_rays, n_samples, dist, t_min, rays_o, rays_d, sdf_dense, pts, mask, zval):
    _lib.call('pp_sdf_first_crossing', _f(sdf), _i(ray_start), _i(step_k), n_rays, n_samples, float(dist), _f(t_min),
              _f(rays_o), _f(rays_d), _f(sdf_dense), _f(pts), _ptr(mask, torch.uint8), _f(zval), _stream())


def sdf_crossing_dense_bwd(sc, sdf_grid, rays_o, rays_d, t_min, jitter, n_rays, n_samples, dist, sdf_dense, g_pts, g_sdf_dense,
                           g_rays_o, g_rays_d, g_t_min):
    _lib.call('pp_sdf_crossing_dense_bwd', ctypes.byref(sc), _f(sdf_grid), _f(rays_o), _f(rays_d), _f(t_min), _f(jitter),
              n_rays, n_samples, float(dist), _f(sdf_dense), _f(g_pts), _f(g_sdf_dense), _f(g_rays_o), _f(g_rays_d),
              _f(g_t_min), _stream())


def feat_generic_fwd(sc, k0_cl, pts, viewdirs, ray_id, gradient, pe_w, sel, k0_skip, ld, count, capacity, feat, k0_raw):
    _lib.call('pp_feat_generic_fwd', ctypes.byref(sc), _f(k0_cl), _f(pts), _f(viewdirs), _i(ray_id), _f(gradient), _f(pe_w),
              _ptr(sel, torch.uint8), int(k0_skip), int(ld), _i(count), capacity, _f(feat), _f(k0_raw), _stream())


def feat_generic_bwd_k0(sc, pts, sel, k0_skip, ld, count, capacity, feat_grad, k0_raw_grad, k0_grad_cl):
    _lib.call('pp_feat_generic_bwd_k0', ctypes.byref(sc), _f(pts), _ptr(sel, torch.uint8), int(k0_skip), int(ld), _i(count),
              capacity, _f(feat_grad), _f(k0_raw_grad), _f(k0_grad_cl), _stream())


def mlp_workspace(in_ld, n_gemm, capacity):
    """-> (acts, scratch) in floats for mlp_fwd / mlp_bwd of this shape, from the library's workspace query."""
    a, s = ctypes.c_int64(), ctypes.c_int64()
    _lib.call('pp_mlp_workspace', int(in_ld), int(n_gemm), int(capacity), ctypes.byref(a), ctypes.byref(s))
    return a.value, s.value


def mlp_fwd(params, feat, in_ld, n_gemm, count, capacity, logit_add, logit_add_ld, acts, out, ctx=None):
    _lib.call('pp_mlp_fwd', _f(params), _f(feat), int(in_ld), int(n_gemm), _i(count), capacity, _f(logit_add),
              int(logit_add_ld), _f(acts), _f(out), _h(ctx), _stream())


def mlp_bwd(params, feat, in_ld, n_gemm, acts, out, out_grad, count, capacity, scratch, params_grad, feat_grad,
            logit_add_grad, logit_add_ld, ctx=None):
    _lib.call('pp_mlp_bwd', _f(params), _f(feat), int(in_ld), int(n_gemm), _f(acts), _f(out), _f(out_grad), _i(count),
              capacity, _f(scratch), _f(params_grad), _f(feat_grad), _f(logit_add_grad), int(logit_add_ld), _h(ctx),
              _stream())


def march_dvgo_fwd(alpha, rgb, step_w, ray_start, n_rays, weights, T, alphainv_last, i_end, rgb_acc, cum_weights, depth_acc):
    _lib.call('pp_march_dvgo_fwd', _f(alpha), _f(rgb), _f(step_w), _i(ray_start), n_rays, _f(weights), _f(T),
              _f(alphainv_last), _i(i_end), _f(rgb_acc), _f(cum_weights), _f(depth_acc), _stream())


# ------------------------------------------------------------------------------------------- scene branch (NeRF)
def nerf_layout():
    """Offsets (floats) of {W0,b0,...,W7,b7,wd,bd,R0,br0,R1,br1} in the packed parameter block and its total size."""
    off = (ctypes.c_int64 * 23)()
    _lib.call('pp_nerf_layout', off)
    return list(off)


def nerf_workspace(n_samples, n_rays):
    a, s = ctypes.c_int64(), ctypes.c_int64()
    _lib.call('pp_nerf_workspace', ctypes.c_int64(n_samples), ctypes.c_int64(n_rays), ctypes.byref(a), ctypes.byref(s))
    return a.value, s.value


def nerf_fwd(params, center, ray, depth, bands, count, n_rays, n_samples, acts, rgb_samples, density_samples, ctx=None):
    _lib.call('pp_nerf_fwd', _f(params), _f(center), _f(ray), _f(depth), _f(bands), _i(count), int(n_rays), int(n_samples),
              _f(acts), _f(rgb_samples), _f(density_samples), _h(ctx), _stream())


def nerf_infer_workspace(n_samples, n_rays):
    """Floats of pp_nerf_infer's workspace: 224 per sample + a part that does not depend on the sample count."""
    w = ctypes.c_int64()
    _lib.call('pp_nerf_infer_workspace', ctypes.c_int64(n_samples), ctypes.c_int64(n_rays), ctypes.byref(w))
    return w.value


def nerf_infer(params, center, ray, depth, bands, count, n_rays, n_samples, work, rgb_samples, density_samples, ctx=None):
    """nerf_fwd that keeps no activations (pp_nerf_infer): the same rgb_samples / density_samples bits; `work` of
    nerf_infer_workspace floats; default route only (another one raises PoseProbeError: use nerf_fwd)."""
    R, M = int(n_rays), int(n_rays) * int(n_samples)
    _rows_at_least(R, (center, 3, 'center'), (ray, 3, 'ray'), (depth, int(n_samples), 'depth'))
    _rows_at_least(M, (rgb_samples, 3, 'rgb_samples'), (density_samples, 1, 'density_samples'))
    _rows_at_least(1, (work, nerf_infer_workspace(M, R), 'work'))
    _lib.call('pp_nerf_infer', _f(params), _f(center), _f(ray), _f(depth), _f(bands), _i(count), R, int(n_samples),
              _f(work), _f(rgb_samples), _f(density_samples), _h(ctx), _stream())


def nerf_bwd(params, ray, depth, count, n_rays, n_samples, acts, rgb_samples, g_rgb_samples, g_density_samples, scratch,
             params_grad, g_center, g_ray, ctx=None):
    _lib.call('pp_nerf_bwd', _f(params), _f(ray), _f(depth), _i(count), int(n_rays), int(n_samples), _f(acts), _f(rgb_samples),
              _f(g_rgb_samples), _f(g_density_samples), _f(scratch), _f(params_grad), _f(g_center), _f(g_ray), _h(ctx), _stream())


def nerf_bwd_input(params, ray, depth, count, n_rays, n_samples, acts, rgb_samples, g_rgb_samples, g_density_samples, scratch,
                   g_center, g_ray, ctx=None):
    """nerf_bwd with respect to the rays only (pp_nerf_bwd_input): no parameter gradient is formed or touched; g_center / g_ray
    are the bits nerf_bwd gives."""
    R, M = int(n_rays), int(n_rays) * int(n_samples)
    a, s = nerf_workspace(M, R)
    _rows_at_least(R, (ray, 3, 'ray'), (depth, int(n_samples), 'depth'), (g_center, 3, 'g_center'), (g_ray, 3, 'g_ray'))
    _rows_at_least(M, (rgb_samples, 3, 'rgb_samples'), (g_rgb_samples, 3, 'g_rgb_samples'), (g_density_samples, 1, 'g_density_samples'))
    _rows_at_least(1, (acts, a, 'acts'), (scratch, s, 'scratch'))
    _lib.call('pp_nerf_bwd_input', _f(params), _f(ray), _f(depth), _i(count), R, int(n_samples), _f(acts), _f(rgb_samples),
              _f(g_rgb_samples), _f(g_density_samples), _f(scratch), _f(g_center), _f(g_ray), _h(ctx), _stream())


def nerf_rays_select(c2w, K, ray_idx, H, W, image, center, ray, dir_cam, target):
    """c2w [3,4], K [3,3] (upper-triangular, K[2,2] = 1: the caller checks), ray_idx [N] int32 in [0, H * W), image [H,W,3] ->
    center, ray, dir_cam, target [N,3] (pp_nerf_rays_select), all on the device."""
    N = ray_idx.shape[0]
    if c2w.numel() != 12 or K.numel() != 9 or image.numel() != H * W * 3:
        raise RuntimeError('nerf_rays_select: c2w [3,4], K [3,3] and image [H,W,3] expected')
    _rows_at_least(N, (center, 3, 'center'), (ray, 3, 'ray'), (dir_cam, 3, 'dir_cam'), (target, 3, 'target'))
    _lib.call('pp_nerf_rays_select', _f(c2w), _f(K), _i(ray_idx), int(N), int(H), int(W), _f(image), _f(center), _f(ray),
              _f(dir_cam), _f(target), _stream())


def nerf_mse_loss(pred, label, weight, loss, g_pred):
    """loss[0] = weight * mse_loss(pred, label, mean); g_pred = its gradient (eval.py:853)."""
    n = int(pred.numel())
    _rows_at_least(n, (label, 1, 'label'), (g_pred, 1, 'g_pred'))
    _rows_at_least(1, (loss, 1, 'loss'))
    _lib.call('pp_nerf_mse_loss', _f(pred), _f(label), n, ctypes.c_float(weight), _f(loss), _f(g_pred), _stream())


def nerf_composite_fwd(rgb_samples, density_samples, depth, ray, n_rays, n_samples, white_bg, rgb, depth_out, opacity, weights,
                       all_cumulated, rgb_var, depth_var):
    _lib.call('pp_nerf_composite_fwd', _f(rgb_samples), _f(density_samples), _f(depth), _f(ray), int(n_rays), int(n_samples),
              int(bool(white_bg)), _f(rgb), _f(depth_out), _f(opacity), _f(weights), _f(all_cumulated), _f(rgb_var),
              _f(depth_var), _stream())


def nerf_composite_bwd(rgb_samples, density_samples, depth, ray, weights, n_rays, n_samples, white_bg, g_rgb, g_depth, g_opacity,
                       g_weights, g_rgb_samples, g_density_samples, g_ray):
    _lib.call('pp_nerf_composite_bwd', _f(rgb_samples), _f(density_samples), _f(depth), _f(ray), _f(weights), int(n_rays),
              int(n_samples), int(bool(white_bg)), _f(g_rgb), _f(g_depth), _f(g_opacity), _f(g_weights), _f(g_rgb_samples),
              _f(g_density_samples), _f(g_ray), _stream())


def nerf_band_weights(progress, start, end, l_3d, l_view, bands):
    _lib.call('pp_nerf_band_weights', _f(progress), ctypes.c_float(start), ctypes.c_float(float(end) - float(start)), int(l_3d), int(l_view), _f(bands),
              _stream())


def nerf_huber_loss(pred, label, delta, weight, loss, g_pred):
    """loss[0] = weight * huber(pred, label, delta, mean); g_pred = its gradient (base_losses.py:155-156)."""
    _lib.call('pp_nerf_huber_loss', _f(pred), _f(label), int(pred.numel()), ctypes.c_float(delta), ctypes.c_float(weight), _f(loss),
              _f(g_pred), _stream())


def nerf_corres_loss(depth0, depth1, pix_self, pix_other, conf, K_self, K_other, w2c_self, w2c_other, pixel_check, pixel_thresh,
                     depth_check, depth_thresh, weight, loss, g_depth0, g_depth1, g_w2c):
    """depth0 / depth1 (None: one pass) [2M] = [self M | other M]; the rest as pp_nerf_corres_loss (include/poseprobe_hip.h)."""
    M = pix_self.shape[0]
    for t, n, what in ((depth0, 2 * M, 'depth0'), (g_depth0, 2 * M, 'g_depth0'), (pix_other, 2 * M, 'pix_other'),
                       (pix_self, 2 * M, 'pix_self'), (conf, M, 'conf'), (K_self, 9, 'K_self'), (K_other, 9, 'K_other'),
                       (w2c_self, 12, 'w2c_self'), (w2c_other, 12, 'w2c_other'), (g_w2c, 24, 'g_w2c'), (loss, 1, 'loss')):
        if t.numel() < n:
            raise RuntimeError(f'{what} holds {t.numel()} floats, needs {n}')
    if (depth1 is None) != (g_depth1 is None) or (depth1 is not None and min(depth1.numel(), g_depth1.numel()) < 2 * M):
        raise RuntimeError('depth1 / g_depth1: both None or both [2M]')
    _lib.call('pp_nerf_corres_loss', _f(depth0), _f(depth1), int(M), _f(pix_self), _f(pix_other), _f(conf), _f(K_self),
              _f(K_other), _f(w2c_self), _f(w2c_other), int(bool(pixel_check)), ctypes.c_float(pixel_thresh),
              int(bool(depth_check)), ctypes.c_float(depth_thresh), ctypes.c_float(weight), _f(loss), _f(g_depth0), _f(g_depth1),
              _f(g_w2c), _stream())


def nerf_pair_pose_bwd(g_center, g_ray, dir_cam, w2c, g_w2c, view_self, view_other, g_c2w):
    """g_center / g_ray / dir_cam [2M,3] (self rows, then other rows); w2c / g_c2w [V,3,4]; g_w2c [2,3,4] or None."""
    M2, V = g_center.shape[0], w2c.shape[0]
    if M2 % 2 or g_ray.shape[0] != M2 or dir_cam.shape[0] != M2 or g_c2w.shape[0] != V or (g_w2c is not None and g_w2c.numel() < 24):
        raise RuntimeError('nerf_pair_pose_bwd: inconsistent shapes')
    _lib.call('pp_nerf_pair_pose_bwd', _f(g_center), _f(g_ray), _f(dir_cam), int(M2 // 2), _f(w2c), _f(g_w2c), int(V),
              int(view_self), int(view_other), _f(g_c2w), _stream())


# ------------------------------------------------------------------------------------------- object branch: reprojection terms
def _rows_at_least(n, *named):
    for t, width, what in named:
        if t is not None and t.numel() < n * width:
            raise RuntimeError(f'{what} holds {t.numel()} elements, needs {n * width}')


def reproj_rays(sc, own, pix, n_rows, intr, c2w, rays_o, rays_d, viewdirs):
    """own [n_rows] int32, pix [n_rows,2] -> rays_o / rays_d / viewdirs [capacity,3]; rows from n_rows on miss the box."""
    cap = rays_o.shape[0]
    _rows_at_least(n_rows, (own, 1, 'own'), (pix, 2, 'pix'))
    _rows_at_least(cap, (rays_d, 3, 'rays_d'), (viewdirs, 3, 'viewdirs'))
    _lib.call('pp_reproj_rays', ctypes.byref(sc), _i(own), _f(pix), int(n_rows), int(cap), _f(intr), _f(c2w), c2w.shape[0],
              _f(rays_o), _f(rays_d), _f(viewdirs), _stream())


def reproj_dense_pts(sc, rays_o, rays_d, t_min, jitter, pts):
    """pts [N * n_samples, 3]: the dense sample positions of the zero-crossing query."""
    N = rays_o.shape[0]
    _rows_at_least(N, (rays_d, 3, 'rays_d'), (t_min, 1, 't_min'), (jitter, 1, 'jitter'), (pts, 3 * sc.n_samples, 'pts'))
    _lib.call('pp_reproj_dense_pts', ctypes.byref(sc), _f(rays_o), _f(rays_d), _f(t_min), _f(jitter), int(N), _f(pts), _stream())


def reproj_loss(render, n_rows, other, match, conf, rays_o, rays_d, p, hit, t_min, acc, intr, w2c, centre, half_diagonal, nl,
                pixel_thre, w_near, w_proj, scale, terms, g_p, g_depth, g_o, g_d, g_w2c):
    """See pp_reproj_loss (include/poseprobe_hip.h).  centre: three Python floats; pixel_thre None = no pixel filter.  The per-row
    outputs define the capacity (g_p [capacity,3])."""
    cap, V = g_p.shape[0], w2c.shape[0]
    _rows_at_least(n_rows, (other, 1, 'other'), (match, 2, 'match'), (conf, 1, 'conf'), (rays_o, 3, 'rays_o'),
                   (rays_d, 3, 'rays_d'), (p, 3, 'p'), (hit, 1, 'hit'), (t_min, 1, 't_min'), (acc, 1, 'acc'))
    _rows_at_least(cap, (g_depth, 1, 'g_depth'), (g_o, 3, 'g_o'), (g_d, 3, 'g_d'))
    _rows_at_least(V, (intr, 4, 'intr'), (g_w2c, 12, 'g_w2c'))
    _rows_at_least(3, (terms, 1, 'terms'))
    _lib.call('pp_reproj_loss', int(bool(render)), int(n_rows), int(cap), _i(other), _f(match), _f(conf), _f(rays_o), _f(rays_d),
              _f(p), _u8(hit), _f(t_min), _f(acc), _f(intr), _f(w2c), int(V), float(centre[0]), float(centre[1]),
              float(centre[2]), float(half_diagonal), float(nl), int(pixel_thre is not None),
              float(0.0 if pixel_thre is None else pixel_thre), float(w_near), float(w_proj), float(scale), _f(terms), _f(g_p),
              _f(g_depth), _f(g_o), _f(g_d), _f(g_w2c), _stream())


def reproj_pose_fold(sc, own, pix, n_rows, intr, c2w, w2c, rays_o, rays_d, g_o, g_d, g_viewdirs, g_t_min, g_w2c, g_c2w):
    """Per-row ray gradients of the rows' own views (+ the direct w2c gradient, or None) -> g_c2w [V,3,4], overwritten."""
    V = c2w.shape[0]
    _rows_at_least(n_rows, (own, 1, 'own'), (pix, 2, 'pix'), (rays_o, 3, 'rays_o'), (rays_d, 3, 'rays_d'), (g_o, 3, 'g_o'),
                   (g_d, 3, 'g_d'), (g_viewdirs, 3, 'g_viewdirs'), (g_t_min, 1, 'g_t_min'))
    _rows_at_least(V, (intr, 4, 'intr'), (w2c, 12, 'w2c'), (g_w2c, 12, 'g_w2c'), (g_c2w, 12, 'g_c2w'))
    _lib.call('pp_reproj_pose_fold', ctypes.byref(sc), _i(own), _f(pix), int(n_rows), _f(intr), _f(c2w), _f(w2c), int(V),
              _f(rays_o), _f(rays_d), _f(g_o), _f(g_d), _f(g_viewdirs), _f(g_t_min), _f(g_w2c), _f(g_c2w), _stream())


# ------------------------------------------------------------------------------------------- object branch: surface-projection feature loss
FEATPROJ_MAX_LAYERS = 4
FEATPROJ_MAX_CHANNELS = 512


def featproj_reproject(n_rows, view_j, rays_o, rays_d, t_min, acc, intr, w2c, nl, own_ref, pix_ref):
    """Surface points of query A -> pix_ref [capacity,2], own_ref [capacity] int32: the rows of query B (pp_featproj_reproject)."""
    cap, V = pix_ref.shape[0], w2c.shape[0]
    _rows_at_least(n_rows, (rays_o, 3, 'rays_o'), (rays_d, 3, 'rays_d'), (t_min, 1, 't_min'), (acc, 1, 'acc'))
    _rows_at_least(cap, (own_ref, 1, 'own_ref'), (pix_ref, 2, 'pix_ref'))
    _rows_at_least(V, (intr, 4, 'intr'))
    _lib.call('pp_featproj_reproject', int(n_rows), int(cap), int(view_j), _f(rays_o), _f(rays_d), _f(t_min), _f(acc), _f(intr),
              _f(w2c), int(V), float(nl), _i(own_ref), _f(pix_ref), _stream())


def featproj_loss(n_rows, view_i, view_j, rays_o, rays_d, t_min, acc, ref_rays_o, ref_rays_d, ref_t_min, ref_acc, intr, w2c, nl,
                  voxel_size, H, W, layers, weight, scale, terms, valid, cosv, g_q, g_depth, g_o, g_d, g_w2c):
    """See pp_featproj_loss (include/poseprobe_hip.h).  layers: up to four channels-last [V,h,w,C] fp32 maps.  The per-row outputs
    define the capacity (g_o [capacity,3])."""
    cap, V, L = g_o.shape[0], w2c.shape[0], len(layers)
    if not 1 <= L <= FEATPROJ_MAX_LAYERS:
        raise ValueError(f'{L} feature layers: need 1 to {FEATPROJ_MAX_LAYERS}')
    for t in layers:
        if t.dim() != 4 or t.shape[0] != V:
            raise RuntimeError(f'a feature layer must be [n_views = {V}, h, w, C], got {tuple(t.shape)}')
    _rows_at_least(n_rows, (rays_o, 3, 'rays_o'), (rays_d, 3, 'rays_d'), (t_min, 1, 't_min'), (acc, 1, 'acc'),
                   (ref_rays_o, 3, 'ref_rays_o'), (ref_rays_d, 3, 'ref_rays_d'), (ref_t_min, 1, 'ref_t_min'), (ref_acc, 1, 'ref_acc'))
    _rows_at_least(cap, (valid, 1, 'valid'), (cosv, L, 'cosv'), (g_q, 6, 'g_q'), (g_depth, 1, 'g_depth'), (g_d, 3, 'g_d'))
    _rows_at_least(V, (intr, 4, 'intr'), (g_w2c, 12, 'g_w2c'))
    _rows_at_least(2 + FEATPROJ_MAX_LAYERS, (terms, 1, 'terms'))
    dims = (ctypes.c_int32 * (3 * L))(*[int(x) for t in layers for x in (t.shape[3], t.shape[1], t.shape[2])])
    feats = [_f(t, 'feature layer') for t in layers] + [None] * (FEATPROJ_MAX_LAYERS - L)
    _lib.call('pp_featproj_loss', int(n_rows), int(cap), int(view_i), int(view_j), _f(rays_o), _f(rays_d), _f(t_min), _f(acc),
              _f(ref_rays_o), _f(ref_rays_d), _f(ref_t_min), _f(ref_acc), _f(intr), _f(w2c), int(V), float(nl), float(voxel_size),
              int(H), int(W), L, *feats, ctypes.cast(dims, ctypes.c_void_p), float(weight), float(scale), _f(terms), _u8(valid),
              _f(cosv), _f(g_q), _f(g_depth), _f(g_o), _f(g_d), _f(g_w2c), _stream())


# ------------------------------------------------------------------------------------------- scene branch: ordered step
def nerf_ordered_workspace():
    """Bytes of the workspace of the scene branch's ordered weight-gradient flush (pp_nerf_ordered_workspace): 512 slots of
    64 KB + 512 B, whatever the shapes."""
    b = ctypes.c_int64()
    _lib.call('pp_nerf_ordered_workspace', ctypes.byref(b))
    return b.value


def nerf_ordered_attach(ctx, work):
    """Record `work` (uint8 tensor of nerf_ordered_workspace() bytes; None = detach) in `ctx` (an _lib.Context, required):
    nerf_bwd calls handed this context then add the weight gradients up in a fixed order instead of by float atomics.  The
    caller keeps `work` alive while such calls are in flight; contexts whose calls share a stream may share one workspace."""
    if ctx is None:
        raise ValueError('nerf_ordered_attach needs a context of its own (the default context is shared by everybody)')
    _lib.call('pp_nerf_ordered_attach', ctx.handle, _u8(work), 0 if work is None else int(work.numel()))


def nerf_c2w_fold(g_ray, g_center, dir_cam, g_c2w):
    """g_ray / g_center / dir_cam [V, N, 3] -> g_c2w [V_total, 3, 4] = [sum g_ray (x) dir_cam | sum g_center] in a fixed order
    (rows V .. V_total - 1: zeros)."""
    V, N = g_ray.shape[:2]
    if tuple(g_ray.shape) != (V, N, 3) or g_center.shape != g_ray.shape or dir_cam.shape != g_ray.shape or \
            g_c2w.dim() != 3 or tuple(g_c2w.shape[1:]) != (3, 4) or g_c2w.shape[0] < V:
        raise RuntimeError('nerf_c2w_fold: inconsistent shapes')
    _lib.call('pp_nerf_c2w_fold', _f(g_ray), _f(g_center), _f(dir_cam), int(V), int(N), int(g_c2w.shape[0]), _f(g_c2w), _stream())


def nerf_sample_pdf(weights, depth, grid, n_fine, depth_range, depth_out):
    """weights, depth [R, S]; grid [n_fine + 1] (shared) or [R, n_fine + 1] -> depth_out [R, S + n_fine]: the coarse depths and the
    inverse-transform samples of the coarse weights, ascending (bg_nerf.sample_depth_from_pdf + cat + sort in one launch)."""
    R, S = weights.shape
    per_ray = grid.dim() == 2
    if depth.shape != weights.shape or tuple(grid.shape) != ((R, n_fine + 1) if per_ray else (n_fine + 1,)) or \
            tuple(depth_out.shape) != (R, S + n_fine):
        raise RuntimeError('nerf_sample_pdf: inconsistent shapes')
    _lib.call('pp_nerf_sample_pdf', _f(weights), _f(depth), _f(grid), int(per_ray), int(R), int(S), int(n_fine),
              ctypes.c_float(depth_range[0]), ctypes.c_float(depth_range[1]), _f(depth_out), _stream())


# ------------------------------------------------------------------------------------------- mesh extraction
def mc_table():
    """The 256-case triangle table of the marching-cubes kernels as an int32 [256, 16] numpy array (rows of edge ids in triples,
    -1 terminated; numbering in include/poseprobe_hip.h).  A pure host call: needs no GPU."""
    t = np.empty((256, 16), dtype=np.int32)
    _lib.call('pp_mc_table', t.ctypes.data_as(ctypes.c_void_p))
    return t


def mc_workspace(X, Y, Z):
    """Bytes of device workspace pp_mc_count / pp_mc_emit need for an [X, Y, Z] lattice."""
    b = ctypes.c_int64()
    _lib.call('pp_mc_workspace', int(X), int(Y), int(Z), ctypes.byref(b))
    return b.value


def _mc_lattice(u):
    if u is not None and u.dim() != 3:
        raise RuntimeError('u must be a [X, Y, Z] lattice')
    return (0, 0, 0) if u is None else tuple(int(s) for s in u.shape)


def mc_count(u, threshold, work, counts):
    """Classify the lattice u [X,Y,Z] into `work` (uint8, mc_workspace bytes); counts [2] int32 <- (vertices, triangles)."""
    X, Y, Z = _mc_lattice(u)
    _lib.call('pp_mc_count', _f(u, 'u'), X, Y, Z, ctypes.c_float(threshold), _u8(work, 'work'),
              0 if work is None else int(work.numel()), _i(counts, 'counts'), _stream())


def mc_emit(u, threshold, work, vertices, n_vertices, triangles, n_triangles):
    """After mc_count with the same u, threshold and work: rows [0, n_vertices) of vertices [.,3] fp32 and [0, n_triangles) of
    triangles [.,3] int32."""
    X, Y, Z = _mc_lattice(u)
    for t, n, name in ((vertices, n_vertices, 'vertices'), (triangles, n_triangles, 'triangles')):
        if t is not None and t.numel() < 3 * int(n):
            raise RuntimeError(f'{name}: {t.numel() // 3} rows, {int(n)} to be written')
    _lib.call('pp_mc_emit', _f(u, 'u'), X, Y, Z, ctypes.c_float(threshold), _u8(work, 'work'),
              0 if work is None else int(work.numel()), _f(vertices, 'vertices'), int(n_vertices), _i(triangles, 'triangles'),
              int(n_triangles), _stream())


def vertex_feat(sc, sdf_grid, sdf_ab, k0_cl, pts, warp_out, pe_w, n, normal, feat):
    """Rows [0, n) of normal [.,3] and of feat [.,64] (the rgbnet's input, view direction = -normal) for the vertices pts [.,3]
    (pp_vertex_feat); warp_out [.,16] = warp_fwd's rows of these points, None = the plain template.  n = 0 launches nothing."""
    n = int(n)
    voxels = int(sc.size[0]) * int(sc.size[1]) * int(sc.size[2])
    _rows_at_least(n, (pts, 3, 'pts'), (warp_out, 16, 'warp_out'), (normal, 3, 'normal'), (feat, FEAT_LD, 'feat'))
    _rows_at_least(voxels, (sdf_grid, 1, 'sdf_grid'), (k0_cl, int(sc.k0_dim), 'k0_cl'))
    _rows_at_least(1, (sdf_ab, 2, 'sdf_ab'), (pe_w, int(sc.pos_pe) + int(sc.view_pe), 'pe_w'))
    _lib.call('pp_vertex_feat', ctypes.byref(sc), _f(sdf_grid, 'sdf_grid'), _f(sdf_ab, 'sdf_ab'), _f(k0_cl, 'k0_cl'), _f(pts, 'pts'),
              _f(warp_out, 'warp_out'), _f(pe_w, 'pe_w'), n, _f(normal, 'normal'), _f(feat, 'feat'), _stream())


# ------------------------------------------------------------------------------------------- mesh cleaning (connected components)
def cc_workspace(n_vertices):
    """Bytes of device workspace pp_cc_rounds needs for n_vertices vertices (a pure host call)."""
    b = ctypes.c_int64()
    _lib.call('pp_cc_workspace', int(n_vertices), ctypes.byref(b))
    return b.value


def _cc_mesh(triangles, n_vertices, *per_vertex):
    if triangles is not None and (triangles.dim() != 2 or triangles.shape[1] != 3):
        raise RuntimeError('triangles must be [.,3]')
    Nv = int(n_vertices)
    for t, name in per_vertex:
        if t is not None and t.numel() != Nv:
            raise RuntimeError(f'{name}: {t.numel()} elements, {Nv} expected')
    return 0 if triangles is None else int(triangles.shape[0]), Nv


def cc_rounds(triangles, n_vertices, first_round, n_rounds, labels, work, changed):
    """Rounds first_round .. first_round + n_rounds - 1 of the component labelling of triangles [Nt,3] int32 (first_round = 0
    initialises labels [Nv] int32 and work); changed [n_rounds] int32 <- 1 where that round changed a label."""
    Nt, Nv = _cc_mesh(triangles, n_vertices, (labels, 'labels'))
    if changed is not None and changed.numel() < int(n_rounds):
        raise RuntimeError(f'changed: {changed.numel()} elements, {int(n_rounds)} expected')
    _lib.call('pp_cc_rounds', _i(triangles, 'triangles'), Nt, Nv, int(first_round), int(n_rounds), _i(labels, 'labels'),
              _u8(work, 'work'), 0 if work is None else int(work.numel()), _i(changed, 'changed'), _stream())


def cc_count(labels, triangles, vertex_counts, triangle_counts):
    """labels [Nv] of cc_rounds at its fixpoint -> vertex_counts, triangle_counts [Nv] int32 indexed by root (0 elsewhere)."""
    Nt, Nv = _cc_mesh(triangles, 0 if labels is None else labels.numel(), (vertex_counts, 'vertex_counts'),
                      (triangle_counts, 'triangle_counts'))
    _lib.call('pp_cc_count', _i(labels, 'labels'), Nv, _i(triangles, 'triangles'), Nt, _i(vertex_counts, 'vertex_counts'),
              _i(triangle_counts, 'triangle_counts'), _stream())


def cc_keep_masks(labels, triangles, root_keep, vertex_keep, triangle_keep):
    """root_keep [Nv] uint8 marks the roots to keep -> vertex_keep [Nv], triangle_keep [Nt] int32 (1 = kept)."""
    Nt, Nv = _cc_mesh(triangles, 0 if labels is None else labels.numel(), (root_keep, 'root_keep'), (vertex_keep, 'vertex_keep'))
    if triangle_keep is not None and triangle_keep.numel() != Nt:
        raise RuntimeError(f'triangle_keep: {triangle_keep.numel()} elements, {Nt} expected')
    _lib.call('pp_cc_keep_masks', _i(labels, 'labels'), Nv, _i(triangles, 'triangles'), Nt, _u8(root_keep, 'root_keep'),
              _i(vertex_keep, 'vertex_keep'), _i(triangle_keep, 'triangle_keep'), _stream())


def cc_compact(vertices, triangles, vertex_scan, triangle_scan, out_vertices, out_index, out_triangles):
    """vertex_scan [Nv] / triangle_scan [Nt] int32 = inclusive scans of cc_keep_masks' masks -> the kept rows, in order, in
    out_vertices [Nv',3], out_index [Nv'] int32 (old indices) and out_triangles [Nt',3] int32 (renumbered)."""
    if vertices is not None and (vertices.dim() != 2 or vertices.shape[1] != 3):
        raise RuntimeError('vertices must be [.,3]')
    Nt, Nv = _cc_mesh(triangles, 0 if vertices is None else vertices.shape[0], (vertex_scan, 'vertex_scan'))
    if triangle_scan is not None and triangle_scan.numel() != Nt:
        raise RuntimeError(f'triangle_scan: {triangle_scan.numel()} elements, {Nt} expected')
    for t, name in ((out_vertices, 'out_vertices'), (out_triangles, 'out_triangles')):
        if t.dim() != 2 or t.shape[1] != 3:
            raise RuntimeError(f'{name} must be [.,3]')
    if out_index.numel() != out_vertices.shape[0]:
        raise RuntimeError(f'out_index: {out_index.numel()} elements, {out_vertices.shape[0]} expected')
    _lib.call('pp_cc_compact', _f(vertices, 'vertices'), _i(triangles, 'triangles'), _i(vertex_scan, 'vertex_scan'),
              _i(triangle_scan, 'triangle_scan'), Nv, Nt, _f(out_vertices, 'out_vertices'), _i(out_index, 'out_index'),
              _i(out_triangles, 'out_triangles'), int(out_vertices.shape[0]), int(out_triangles.shape[0]), _stream())


# ------------------------------------------------------------------------------------------- pose initialisation (PnP-RANSAC)
def pnp_workspace(P, H):
    """Bytes of device workspace pp_pnp_ransac needs for P rows and H hypotheses (a pure host call)."""
    b = ctypes.c_int64()
    _lib.call('pp_pnp_workspace', int(P), int(H), ctypes.byref(b))
    return b.value


def pnp_workspace_views(work, H):
    """(poses [H,3,4] float64, flags [H] int32, counts [H] int32) as views of a workspace pnp_ransac has filled: what every
    hypothesis came to (layout in include/poseprobe_hip.h); counts is -1 where the hypothesis is invalid."""
    r = lambda n: (n + 255) // 256 * 256
    H = int(H)
    o1 = r(96 * H)
    o2 = o1 + r(4 * H)
    return (work[:96 * H].view(torch.float64).view(H, 3, 4), work[o1:o1 + 4 * H].view(torch.int32),
            work[o2:o2 + 4 * H].view(torch.int32))


def pnp_ransac(world, pix, valid, intr, samples, reproj_error, refine_iters, min_inliers, fallback, work, w2c, inliers, info):
    """world [P,3], pix [P,2], valid [P] uint8 or None, intr [4] (fx, fy, cx, cy), samples [H,4] int32, fallback [3,4] ->
    w2c [3,4], inliers [P] uint8, info [2] int32 = (inlier count, winning hypothesis) or the fallback pose, zeros and (0, -1).
    Three launches on the current stream; nothing is read back."""
    P = 0 if world is None else int(world.shape[0])
    H = 0 if samples is None else int(samples.shape[0])
    for t, n, name in ((world, 3 * P, 'world'), (pix, 2 * P, 'pix'), (valid, P, 'valid'), (intr, 4, 'intr'), (samples, 4 * H, 'samples'),
                       (fallback, 12, 'fallback'), (w2c, 12, 'w2c'), (inliers, P, 'inliers'), (info, 2, 'info')):
        if t is not None and t.numel() != n:
            raise RuntimeError(f'{name}: {t.numel()} elements, {n} expected')
    _lib.call('pp_pnp_ransac', _f(world, 'world'), _f(pix, 'pix'), _u8(valid, 'valid'), P, _f(intr, 'intr'), _i(samples, 'samples'), H,
              ctypes.c_float(reproj_error), int(refine_iters), int(min_inliers), _f(fallback, 'fallback'), _u8(work, 'work'),
              0 if work is None else int(work.numel()), _f(w2c, 'w2c'), _u8(inliers, 'inliers'), _i(info, 'info'), _stream())


# ------------------------------------------------------------------------------------------- mesh evaluation (DTU Chamfer distance)
def _dtu_mesh(vertices, triangles):
    for t, name in ((vertices, 'vertices'), (triangles, 'triangles')):
        if t is not None and (t.dim() != 2 or t.shape[1] != 3):
            raise RuntimeError(f'{name} must be [.,3]')
    return (0 if vertices is None else int(vertices.shape[0])), (0 if triangles is None else int(triangles.shape[0]))


def dtu_sample_count(vertices, triangles, thresh, counts):
    """vertices [V,3] float64, triangles [T,3] int32 -> counts [T] int64: the sampled points of every triangle."""
    V, T = _dtu_mesh(vertices, triangles)
    if counts is not None and counts.numel() != T:
        raise RuntimeError(f'counts: {counts.numel()} elements, {T} expected')
    _lib.call('pp_dtu_sample_count', _ptr(vertices, torch.float64, 'vertices'), V, _i(triangles, 'triangles'), T, ctypes.c_double(thresh),
              _ptr(counts, torch.int64, 'counts'), _stream())


def dtu_sample_emit(vertices, triangles, thresh, offsets, points, n_points):
    """After dtu_sample_count: offsets [T] int64 = the exclusive scan of the counts -> rows [0, n_points) of points [.,3] fp32."""
    V, T = _dtu_mesh(vertices, triangles)
    if offsets is not None and offsets.numel() != T:
        raise RuntimeError(f'offsets: {offsets.numel()} elements, {T} expected')
    if points is not None and points.numel() < 3 * int(n_points):
        raise RuntimeError(f'points: {points.numel() // 3} rows, {int(n_points)} to be written')
    _lib.call('pp_dtu_sample_emit', _ptr(vertices, torch.float64, 'vertices'), V, _i(triangles, 'triangles'), T, ctypes.c_double(thresh),
              _ptr(offsets, torch.int64, 'offsets'), _f(points, 'points'), int(n_points), _stream())


def _dtu_grid(grid):
    """grid = (origin [3], edge, cells [3]) -> the seven scalars of the C ABI."""
    o, edge, n = grid
    return (ctypes.c_float(o[0]), ctypes.c_float(o[1]), ctypes.c_float(o[2]), ctypes.c_float(edge), int(n[0]), int(n[1]), int(n[2]))


def _dtu_rows(t, name):
    if t is not None and (t.dim() != 2 or t.shape[1] != 3):
        raise RuntimeError(f'{name} must be [.,3]')
    return 0 if t is None else int(t.shape[0])


def dtu_cell_keys(points, grid, keys):
    """points [N,3] fp32 -> keys [N] int64: (x ny + y) nz + z of the point's cell in grid = (origin, edge, cells)."""
    N = _dtu_rows(points, 'points')
    if keys is not None and keys.numel() != N:
        raise RuntimeError(f'keys: {keys.numel()} elements, {N} expected')
    _lib.call('pp_dtu_cell_keys', _f(points, 'points'), N, *_dtu_grid(grid), _ptr(keys, torch.int64, 'keys'), _stream())


def dtu_thin_workspace(N):
    """Bytes of device workspace pp_dtu_thin_rounds needs for N points (a pure host call)."""
    b = ctypes.c_int64()
    _lib.call('pp_dtu_thin_workspace', int(N), ctypes.byref(b))
    return b.value


def dtu_thin_state(work, N, rounds_done):
    """The state bytes [N] (0 undecided, 1 kept, 2 removed; in key order) that `rounds_done` rounds have left in the workspace."""
    off = (rounds_done & 1) * ((int(N) + 255) // 256 * 256)
    return work[off:off + int(N)]


def _dtu_sorted(points, keys, order):
    N = _dtu_rows(points, 'points')
    for t, name in ((keys, 'keys'), (order, 'order')):
        if t is not None and t.numel() != N:
            raise RuntimeError(f'{name}: {t.numel()} elements, {N} expected')
    return N


def dtu_thin_rounds(points, keys, order, grid, radius, first_round, n_rounds, work, undecided):
    """Rounds first_round .. first_round + n_rounds - 1 of the radius thinning on points sorted by key (order [N] int32 = their
    indices before sorting); undecided [n_rounds] int32 <- 1 where a point is still undecided after that round."""
    N = _dtu_sorted(points, keys, order)
    if undecided is not None and undecided.numel() < int(n_rounds):
        raise RuntimeError(f'undecided: {undecided.numel()} elements, {int(n_rounds)} expected')
    _lib.call('pp_dtu_thin_rounds', _f(points, 'points'), _ptr(keys, torch.int64, 'keys'), _i(order, 'order'), N, *_dtu_grid(grid),
              ctypes.c_float(radius), int(first_round), int(n_rounds), _u8(work, 'work'), 0 if work is None else int(work.numel()),
              _i(undecided, 'undecided'), _stream())


def dtu_nearest(queries, points, keys, order, grid, max_dist, d2, idx):
    """queries [Q,3]; points sorted by key with keys and order -> d2 [Q] fp32, idx [Q] int32 (in `order` numbering) of the exact
    nearest point, ties to the lowest index; (inf, -1) beyond max_dist."""
    Q = _dtu_rows(queries, 'queries')
    P = _dtu_sorted(points, keys, order)
    for t, name in ((d2, 'd2'), (idx, 'idx')):
        if t is not None and t.numel() != Q:
            raise RuntimeError(f'{name}: {t.numel()} elements, {Q} expected')
    _lib.call('pp_dtu_nearest', _f(queries, 'queries'), Q, _f(points, 'points'), _ptr(keys, torch.int64, 'keys'), _i(order, 'order'), P,
              *_dtu_grid(grid), ctypes.c_float(max_dist), _f(d2, 'd2'), _i(idx, 'idx'), _stream())


# ------------------------------------------------------------------------------------------- mesh -> signed distance grid
def _msdf_mesh(vertices, triangles):
    for t, name in ((vertices, 'vertices'), (triangles, 'triangles')):
        if t is not None and (t.dim() != 2 or t.shape[1] != 3):
            raise RuntimeError(f'{name} must be [.,3]')
    return (0 if vertices is None else int(vertices.shape[0])), (0 if triangles is None else int(triangles.shape[0]))


def _msdf_axes(xs, ys, zs):
    for t, name in ((xs, 'xs'), (ys, 'ys'), (zs, 'zs')):
        if t is not None and t.dim() != 1:
            raise RuntimeError(f'{name} must be a vector')
    return tuple(0 if t is None else int(t.numel()) for t in (xs, ys, zs))


def msdf_bin_count(vertices, triangles, grid, counts):
    """vertices [V,3] fp32, triangles [T,3] int32 -> counts [T] int64: the cells of grid = (origin, edge, cells) every triangle's
    padded bounding box overlaps."""
    V, T = _msdf_mesh(vertices, triangles)
    if counts is not None and counts.numel() != T:
        raise RuntimeError(f'counts: {counts.numel()} elements, {T} expected')
    _lib.call('pp_msdf_bin_count', _f(vertices, 'vertices'), V, _i(triangles, 'triangles'), T, *_dtu_grid(grid),
              _ptr(counts, torch.int64, 'counts'), _stream())


def msdf_bin_emit(vertices, triangles, grid, offsets, keys, tris, n_pairs):
    """After msdf_bin_count: offsets [T] int64 = the exclusive scan of the counts -> the n_pairs (cell key, triangle) pairs in
    keys [n_pairs] int64 and tris [n_pairs] int32, triangle-major."""
    V, T = _msdf_mesh(vertices, triangles)
    if offsets is not None and offsets.numel() != T:
        raise RuntimeError(f'offsets: {offsets.numel()} elements, {T} expected')
    for t, name in ((keys, 'keys'), (tris, 'tris')):
        if t is not None and t.numel() < int(n_pairs):
            raise RuntimeError(f'{name}: {t.numel()} elements, {int(n_pairs)} to be written')
    _lib.call('pp_msdf_bin_emit', _f(vertices, 'vertices'), V, _i(triangles, 'triangles'), T, *_dtu_grid(grid),
              _ptr(offsets, torch.int64, 'offsets'), _ptr(keys, torch.int64, 'keys'), _i(tris, 'tris'), ctypes.c_int64(int(n_pairs)),
              _stream())


def msdf_nearest(queries, axes, vertices, triangles, keys, tris, grid, max_dist, dist, closest, tri, rings=None):
    """queries [Q,3] fp32, or None with axes = (xs [X], ys [Y], zs [Z]): the nodes of that grid, x-major; keys / tris: the pairs
    of msdf_bin_emit sorted by key -> dist [Q], closest [Q,3] fp32 and tri [Q] int32 of the exact nearest point of the mesh,
    ties to the lowest triangle; (inf, NaN, -1) beyond max_dist.  rings [Q] int32 (optional): rings of cells visited."""
    V, T = _msdf_mesh(vertices, triangles)
    xs, ys, zs = (None, None, None) if axes is None else axes
    X, Y, Z = _msdf_axes(xs, ys, zs)
    Q = _dtu_rows(queries, 'queries') if queries is not None else X * Y * Z
    P = 0 if keys is None else int(keys.numel())
    if tris is not None and tris.numel() != P:
        raise RuntimeError(f'tris: {tris.numel()} elements, {P} expected')
    if P > 2 ** 31 - 1:
        raise RuntimeError('more than 2^31 - 1 (cell, triangle) pairs')
    for t, n, name in ((dist, Q, 'dist'), (closest, 3 * Q, 'closest'), (tri, Q, 'tri'), (rings, Q, 'rings')):
        if t is not None and t.numel() != n:
            raise RuntimeError(f'{name}: {t.numel()} elements, {n} expected')
    _lib.call('pp_msdf_nearest', _f(queries, 'queries'), Q, _f(xs, 'xs'), _f(ys, 'ys'), _f(zs, 'zs'), X, Y, Z, _f(vertices, 'vertices'), V,
              _i(triangles, 'triangles'), T, _ptr(keys, torch.int64, 'keys'), _i(tris, 'tris'), P, *_dtu_grid(grid),
              ctypes.c_float(max_dist), _f(dist, 'dist'), _f(closest, 'closest'), _i(tri, 'tri'), _i(rings, 'rings'), _stream())


def msdf_crossing_slots(X, Y, Z):
    """Elements of the int32 crossing counts [X+1,Y,Z] of msdf_crossings (a pure host call)."""
    n = ctypes.c_int64()
    _lib.call('pp_msdf_crossing_slots', int(X), int(Y), int(Z), ctypes.byref(n))
    return n.value


def msdf_crossings(vertices, triangles, xs, ys, zs, counts):
    """counts [X+1,Y,Z] int32 (cleared first) <- per column (j, k) the crossings of the line y = ys[j], z = zs[k] with the mesh,
    in the slot = the number of nodes with xs[i] below the crossing."""
    V, T = _msdf_mesh(vertices, triangles)
    X, Y, Z = _msdf_axes(xs, ys, zs)
    if counts is not None and counts.numel() != (X + 1) * Y * Z:
        raise RuntimeError(f'counts: {counts.numel()} elements, [{X + 1},{Y},{Z}] expected')
    _lib.call('pp_msdf_crossings', _f(vertices, 'vertices'), V, _i(triangles, 'triangles'), T, _f(xs, 'xs'), _f(ys, 'ys'), _f(zs, 'zs'),
              X, Y, Z, _i(counts, 'counts'), _stream())


# ------------------------------------------------------------------------------------------- image score (SSIM)
def ssim_tile():
    """Edge of the output tile one work-group of pp_ssim takes (a pure host call)."""
    t = ctypes.c_int32()
    _lib.call('pp_ssim_tile', ctypes.byref(t))
    return t.value


def ssim_workspace(V, H, W, filter_size):
    """Bytes of device workspace pp_ssim needs for V views of H x W (a pure host call)."""
    b = ctypes.c_int64()
    _lib.call('pp_ssim_workspace', int(V), int(H), int(W), int(filter_size), ctypes.byref(b))
    return b.value


def ssim(img0, img1, max_val, filter_size, filter_sigma, k1, k2, work, out, ssim_map=None):
    """img0, img1 [V,H,W,C] fp32 -> out [V] fp32: the mean SSIM of every view (lib/utils.py rgb_ssim); ssim_map (optional)
    [V, H - fs + 1, W - fs + 1, C] fp32 receives the map.  work: uint8 [ssim_workspace(...)]."""
    V = H = W = C = 0
    if img0 is not None:
        if img0.dim() != 4:
            raise RuntimeError('img0 must be [V,H,W,C]')
        V, H, W, C = (int(x) for x in img0.shape)
    if img1 is not None and img0 is not None and img1.shape != img0.shape:
        raise RuntimeError(f'img1: shape {tuple(img1.shape)}, {tuple(img0.shape)} expected')
    if out is not None and out.numel() != V:
        raise RuntimeError(f'out: {out.numel()} elements, {V} expected')
    fs = int(filter_size)
    if ssim_map is not None and ssim_map.numel() != V * max(H - fs + 1, 0) * max(W - fs + 1, 0) * C:
        raise RuntimeError(f'ssim_map: {ssim_map.numel()} elements, [{V},{H - fs + 1},{W - fs + 1},{C}] expected')
    _lib.call('pp_ssim', _f(img0, 'img0'), _f(img1, 'img1'), V, H, W, C, fs, ctypes.c_double(filter_sigma), ctypes.c_double(max_val),
              ctypes.c_double(k1), ctypes.c_double(k2), _u8(work, 'work'), 0 if work is None else int(work.numel()), _f(out, 'out'),
              _f(ssim_map, 'ssim_map'), _stream())
