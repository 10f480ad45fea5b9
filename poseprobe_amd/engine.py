"""Host-side orchestration of the HIP hot path: workspace, forward chain, hand-derived backward chain and
the fused train step (ray select -> render -> loss -> backward -> optimiser), with zero host syncs.

Mirrors one iteration of the object branch in recon_scene.optimize_increamental
(lib/recon_scene.py:572-606, :648-649, :742-747, :765-771) and Voxurf.forward (lib/voxurf_coarse.py:922-1092).
torch is used for device memory and streams only; every arithmetic step is a kernel of libposeprobe_hip.so.
"""
import contextlib
import math
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import ops

PAD = 64


def _pad(n):
    return (n + PAD - 1) // PAD * PAD


@dataclass
class SceneConfig:
    xyz_min: np.ndarray
    xyz_max: np.ndarray
    num_voxels: int
    stepsize: float = 1.5
    near: float = 0.24
    far: float = 4.8
    bg: float = 0.0
    N_iters: int = 10000
    s_ratio: float = 50.0
    s_start: float = 0.2
    step_start: float = 0.0
    barf_c2f: tuple = (0.6, 1.0)
    posbase_pe: int = 5
    viewbase_pe: int = 1
    k0_dim: int = 12
    out_range: float = 1.0
    inverse_y: bool = True
    sdf_index_exact: bool = False    # True: exact voxel index in the custom SDF sampler above 2^24 voxels (default: the reference's fp32 index)

    def __post_init__(self):
        # identical fp32 arithmetic to Voxurf._set_grid_resolution (voxurf_coarse.py:319-323)
        lo = torch.tensor(np.asarray(self.xyz_min, dtype=np.float32))
        hi = torch.tensor(np.asarray(self.xyz_max, dtype=np.float32))
        vs = ((hi - lo).prod() / self.num_voxels).pow(1 / 3)
        self.voxel_size = float(vs)
        self.world_size = [int(v) for v in ((hi - lo) / vs).long().tolist()]
        self.pp = ops.make_scene(lo.tolist(), hi.tolist(), self.world_size, self.voxel_size, self.stepsize, self.near,
                                 self.far, self.bg, self.out_range, self.k0_dim, self.posbase_pe, self.viewbase_pe,
                                 sdf_index_exact=True if self.sdf_index_exact else None)
        self.n_samples = self.pp.n_samples

    def s_val(self, global_step):
        return 1. / (global_step + self.s_ratio / self.s_start - self.step_start) * self.s_ratio

    def inv_s(self, global_step):
        """1 / s_val as the kernels take it: the fp32 quotient."""
        return float(np.float32(1.0) / np.float32(self.s_val(global_step)))

    @property
    def step_dist(self):
        """Distance between two samples of a ray: the fp32 product stepsize * voxel_size."""
        return float(np.float32(self.stepsize) * np.float32(self.voxel_size))

    def pe_weights(self, progress):
        """BARF c2f weights for xyz (L=posbase_pe) then view (L=viewbase_pe); voxurf_coarse.py:721-732 (fp32 ops)."""
        out = []
        for L in (self.posbase_pe, self.viewbase_pe):
            if self.barf_c2f is None:
                out.append(np.ones(L, dtype=np.float32))
                continue
            start, end = self.barf_c2f
            alpha = (torch.tensor(progress, dtype=torch.float32) - start) / (end - start) * L
            k = torch.arange(L, dtype=torch.float32)
            w = (1 - (alpha - k).clamp_(min=0, max=1).mul_(np.pi).cos_()) / 2
            out.append(w.numpy())
        return np.concatenate(out).astype(np.float32)


def dynamic_weight(w0, w1, it, total):
    """lib/losses.py:30-32"""
    return w0 * math.exp(math.log(w1 / w0) / total * it)


class Workspace:
    """All per-ray / per-sample device buffers for N rays and `capacity` samples (default N*S)."""
    SAMPLER = ('t_min', 't_max', 'ray_start', 'count', 'pts', 'ray_id', 'step_k', 'step')

    def __init__(self, N, capacity, device, sample_capacity=None, backward=True, keep_activations=True, ctx=None, samples=None):
        """samples: {name: tensor} with the SAMPLER buffers of a sampler that has already run: adopted instead of allocated."""
        f = dict(dtype=torch.float32, device=device)
        i = dict(dtype=torch.int32, device=device)
        self.N, self.cap, self.device = N, capacity, device
        e = torch.empty
        # rays
        self.rays_o, self.rays_d, self.viewdirs = e(N, 3, **f), e(N, 3, **f), e(N, 3, **f)
        self.target, self.mask_px = e(N, 3, **f), e(N, **f)
        # samples
        if samples is None:
            self.sample_cap = sc_ = sample_capacity or capacity
            self.t_min, self.t_max = e(N, **f), e(N, **f)
            self.ray_start = torch.zeros(N + 1, **i)
            self.count = torch.zeros(1, **i)
            self.pts, self.ray_id, self.step_k, self.step = e(sc_, 3, **f), e(sc_, **i), e(sc_, **i), e(sc_, **f)
        else:
            for k in self.SAMPLER:
                setattr(self, k, samples[k])
            self.sample_cap = self.pts.shape[0]
        self.wsz = wsz = ops.mlp_workspaces(capacity)      # sizes come from the library (pp_rgbnet_workspace / pp_warp_workspace)
        assert wsz['warp'][0] == 4 * capacity * 4 * 128 and wsz['rgbnet'][0] == 3 * capacity * 128
        # keep_activations=False (inference: nobody will differentiate this pass): the MLP activations are not kept when the forward kernels can run without them
        # (pp_warp_fwd / pp_rgbnet_fwd with acts = NULL: the split-precision kernels, the default): 2.5 KB per sample less to write
        from . import _lib
        octx = _lib.default_context() if ctx is None else ctx          # the context the forward kernels will be called with
        split = octx.get('mlp_split') if octx.get('mlp_fused') else 0
        self.warp_acts = e(4, capacity * 4, 128, **f) if (backward or keep_activations or not split & 1) else None
        self.warp_out = e(capacity, 16, **f)
        self.alpha, self.gradient = e(capacity, **f), e(capacity, 3, **f)
        self.sdf_final, self.sdf_deform, self.grad_deform = e(capacity, **f), e(capacity, **f), e(capacity, 9, **f)
        self.feat = e(capacity, ops.FEAT_LD, **f)
        self.rgb_acts = e(3, capacity, 128, **f) if (backward or keep_activations or not split & 4) else None
        self.rgb = e(capacity, 3, **f)
        self.weights, self.T = e(capacity, **f), e(capacity, **f)
        # ray outputs
        self.alphainv_last, self.i_end = e(N, **f), e(N, **i)
        self.rgb_marched, self.rgb_pre = e(N, 3, **f), e(N, 3, **f)
        self.cum_weights, self.depth_acc = e(N, **f), e(N, **f)
        self.zero_block = torch.zeros(16, **f)          # loss_out[8] | tv_out[1] | mask_sum[1] : one memset per step
        self.loss_out, self.tv_out, self.mask_sum = self.zero_block[:8], self.zero_block[8:9], self.zero_block[9:10]
        if backward:
            self.alloc_backward(True)

    def alloc_backward(self, zero_scratch):
        """Backward buffers (no-op when they exist).  zero_scratch: Ybar of the warp chain (+ transposed weights, layered path) is
        zeroed once, here: inside a lean scope (ops.warp_lean_begin) most of slot 0 is never written, and two engines that went
        through the same steps must hold the same bytes there.  The autograd node's backward runs outside any scope: no memset."""
        if hasattr(self, 'g_alpha'):
            return
        f = dict(dtype=torch.float32, device=self.device)
        e, N, capacity = torch.empty, self.N, self.cap
        self.g_rgbm, self.g_last, self.g_cw = e(N, 3, **f), e(N, **f), e(N, **f)
        self.g_alpha, self.g_rgb = e(capacity, **f), e(capacity, 3, **f)
        self.g_feat = e(capacity, ops.FEAT_LD, **f)
        self.g_gradient, self.g_pts, self.g_view_s = e(capacity, 3, **f), e(capacity, 3, **f), e(capacity, 3, **f)
        self.g_warp_out = e(capacity, 16, **f)
        # no kernel of the product is handed these three; tests/test_hip_step.py takes its shapes from them
        self.g_grad_deform, self.g_corr, self.g_sdf_deform = e(capacity, 9, **f), e(capacity, **f), e(capacity, **f)
        self.scratch = (torch.zeros if zero_scratch else e)(self.wsz['warp'][1], **f)
        self.scratch_rgb = e(self.wsz['rgbnet'][1], **f)   # Ybar of rgbnet: a buffer of its own, so that a lean scope's bytes in
        #                                                              `scratch` depend on the warp chain alone

    def kept_samples(self, backward=False):
        """Buffers of a pass with fast_color_thres > 0 (allocated on first use, kept): see KeptSamples."""
        if not hasattr(self, 'kept'):
            self.kept = KeptSamples(self)
        if backward:
            self.kept.alloc_backward()
        return self.kept


class KeptSamples:
    """The samples of a Workspace whose weight in the first composite exceeds fast_color_thres (ops.keep_compact), at the
    workspace's capacity: every kernel that reads them stops at the device-side `count`.  The attributes the second composite and
    the colour stage read carry the names they have on the Workspace (pts, ray_id, step, alpha, gradient, ray_start, count and
    the four sample gradients), so RenderCore hands one or the other to the same kernels."""

    def __init__(self, ws):
        f = dict(dtype=torch.float32, device=ws.device)
        i = dict(dtype=torch.int32, device=ws.device)
        e, cap, N = torch.empty, ws.cap, ws.N
        self.cap, self.device = cap, ws.device
        self.idx, self.ray_start, self.count = e(cap, **i), torch.zeros(N + 1, **i), torch.zeros(1, **i)
        self.pts, self.ray_id, self.step = e(cap, 3, **f), e(cap, **i), e(cap, **f)
        self.alpha, self.gradient = e(cap, **f), e(cap, 3, **f)
        # the first composite, over every sample: its weights decide the mask and nothing else
        self.weights_all, self.T_all, self.last_all, self.i_end_all = e(cap, **f), e(cap, **f), e(N, **f), e(N, **i)

    def alloc_backward(self):
        if hasattr(self, 'g_alpha'):
            return
        f = dict(dtype=torch.float32, device=self.device)
        e, cap = torch.empty, self.cap
        self.g_alpha, self.g_gradient, self.g_pts, self.g_view_s = e(cap, **f), e(cap, 3, **f), e(cap, 3, **f), e(cap, 3, **f)


class FlatParams:
    """Packed small parameters: [sdf_ab | rgbnet | warp], each segment padded to 64 floats (16-B aligned sub-blocks)."""
    SEG = [('sdf_ab', 2), ('rgbnet', ops.RGBNET_PARAMS), ('warp', ops.WARP_PARAMS)]

    def __init__(self, device, moments=True):
        """moments=False: parameters + gradients only (the drop-in autograd node, whose optimiser lives outside)."""
        self.off, o = {}, 0
        for name, n in self.SEG:
            self.off[name] = (o, n)
            o += _pad(n)
        self.n = o
        z = lambda: torch.zeros(o, dtype=torch.float32, device=device)
        self.data, self.grad = z(), z()
        self.m, self.v = (z(), z()) if moments else (None, None)

    def view(self, name, which='data'):
        o, n = self.off[name]
        return getattr(self, which)[o:o + n]

    # ---- conversion from / to the reference's state_dict tensors -------------------------------------------
    def load_reference(self, sdf_alpha, sdf_beta, rgbnet, warp):
        """rgbnet: 4 x (W[out,in], b) ; warp: 5 x (W, b) in the reference layouts."""
        with torch.no_grad():
            self.view('sdf_ab').copy_(torch.cat([sdf_alpha.reshape(1), sdf_beta.reshape(1)]))
            self.view('rgbnet').copy_(pack_rgbnet(rgbnet).to(self.data.device))
            self.view('warp').copy_(pack_warp(warp).to(self.data.device))

    def export_grads(self):
        g = {'sdf_alpha': self.view('sdf_ab', 'grad')[0:1].clone(), 'sdf_beta': self.view('sdf_ab', 'grad')[1:2].clone()}
        g['rgbnet'] = unpack_rgbnet(self.view('rgbnet', 'grad'))
        g['warp'] = unpack_warp(self.view('warp', 'grad'))
        return g


# The two MLPs inside the flat parameter block, layer by layer: logical (out, in), leading dimension of W as stored (rgbnet layer 0:
# 57 input columns zero-padded to 64), the reference's state_dict prefix.  Each layer is W[out, ld] followed by b[out].
_WARP_PREFIX = 'warp_network.deform_net.net.net.{}.0'
MLP_LAYOUT = {
    'rgbnet': ((128, 57, 64, 'rgbnet.0'), (128, 128, 128, 'rgbnet.2.0'), (128, 128, 128, 'rgbnet.3.0'), (3, 128, 128, 'rgbnet.4')),
    'warp': tuple((o, i, i, _WARP_PREFIX.format(l)) for l, (o, i) in enumerate(((128, 3), (128, 128), (128, 128), (128, 128), (4, 128)))),
}


def _pack(net, layers):
    parts = []
    for (o, i, ld, _), (W, b) in zip(MLP_LAYOUT[net], layers):
        if ld != i:
            Wp = torch.zeros(o, ld, dtype=torch.float32, device=W.device)
            Wp[:, :W.shape[1]] = W
            W = Wp
        parts += [W.reshape(-1), b]
    return torch.cat([p.detach().float() for p in parts])


def _unpack(net, flat):
    at, out = 0, []
    for o, i, ld, _ in MLP_LAYOUT[net]:
        W = flat[at:at + o * ld].reshape(o, ld)[:, :i]; at += o * ld
        b = flat[at:at + o]; at += o
        out.append((W, b))
    return out


def pack_rgbnet(layers, in_dim=57):
    assert in_dim == MLP_LAYOUT['rgbnet'][0][1]              # the table fixes the layout; the argument is kept for callers
    return _pack('rgbnet', layers)


def unpack_rgbnet(flat, in_dim=57):
    assert in_dim == MLP_LAYOUT['rgbnet'][0][1]
    return _unpack('rgbnet', flat)


def pack_warp(layers):
    return _pack('warp', layers)


def unpack_warp(flat):
    return _unpack('warp', flat)


class RenderCore:
    """Forward and backward kernel chains over a Workspace.  Parameters are passed as raw device tensors:
    k0_cl [X,Y,Z,C] (channels-last), sdf [X,Y,Z], flat (FlatParams-like with .view)."""

    def __init__(self, cfg: SceneConfig, ctx=None, ordered=False):
        """ordered: `ctx` (required then) has an ordered-flush workspace attached (ops.ordered_attach) - the fused step's backward
        uses the ordered form of the geometry backward as well (the MLP calls pick the workspace up from the context).
        ctx: the pp_context (ops.Context) every option-dependent kernel of this core is called with; None = the host's
        default context."""
        self.cfg = cfg
        self.ctx = ctx
        self.ordered = bool(ordered)
        if self.ordered and ctx is None:
            raise ValueError('an ordered RenderCore needs its own context (the workspace is attached to it)')

    @contextlib.contextmanager
    def pass_scope(self, flat, pack, lean_ws=None, pack_with=None, join_wgrad=False):
        """One render pass: the MLP weights of `flat` are packed into `pack` HERE, on the pass's stream, and the record is dropped when
        the pass's kernels are enqueued - also when the pass raises.  Every writer of the parameters (the optimiser, a checkpoint
        load, an in-place copy from outside) runs between two scopes, so no kernel can read a pack older than its parameters.
        pack_with: a callable that packs exactly these into `pack` for this context in a launch it shares with other work (the train
        step's ops.step_begin) - called in place of ops.mlp_pack.
        lean_ws: the Workspace whose warp_acts / scratch the pass differentiates through - a lean scope of the warp net, closed with
        the pack record: the forward kernel leaves out the tangent rows of X0, the data-gradient kernel Ybar3, and the
        weight-gradient kernel rebuilds both (option warp_lean).
        join_wgrad (the train step's default path): a join scope of the weight gradients (ops.wgrad_join_begin) inside the lean scope -
        rgbnet_bwd leaves its weight-gradient chain to the launch of warp_bwd / warp_bwd_weights.  Nothing between the
        two may write ws.feat, ws.rgb_acts or ws.scratch_rgb.  A chain nobody took is launched when the scope closes, or dropped
        when the pass raised."""
        lean = lean_ws is not None and lean_ws.warp_acts is not None
        join = bool(join_wgrad) and lean
        raised = True
        try:
            if pack_with is not None:
                pack_with()
            else:
                ops.mlp_pack(flat.view('warp'), flat.view('rgbnet'), pack, self.ctx)
            if lean:
                ops.warp_lean_begin(lean_ws.warp_acts, lean_ws.scratch, flat.view('warp'), self.ctx)
            if join:
                ops.wgrad_join_begin(self.ctx)
            yield
            raised = False
        finally:
            ops.mlp_pack_invalidate(self.ctx)
            if join:
                ops.wgrad_join_end(self.ctx, launch_pending=not raised)
            if lean:
                ops.warp_lean_end(self.ctx)

    # -- forward -------------------------------------------------------------------------------------------
    def sample(self, ws, jitter):
        ops.sample_dense(self.cfg.pp, ws.rays_o, ws.rays_d, jitter, ws.sample_cap, ws.t_min, ws.t_max, ws.ray_start, ws.count,
                         ws.pts, ws.ray_id, ws.step_k, ws.step)

    def forward(self, ws, k0_cl, sdf, sdf_ab, rgbnet_p, warp_p, inv_s, pe_w, step_w=None, before_k0_use=None, normals=None,
                side_by_side=False, composite=True, use_deform=True, color_thres=0.0):
        """use_deform=False: the plain-template geometry (ops.geometry_plain_fwd) - the warp net does not run and ws.sdf_deform /
        ws.grad_deform / ws.warp_out are not written.  color_thres > 0 (fast_color_thres): a first composite over every sample, then
        the second composite and the colour stage on the samples with weight > color_thres (ws.kept, ops.keep_compact).  Both are
        for the drop-in module's passes: not with side_by_side, before_k0_use, step_w or composite=False.  Defaults: no launch differs.
        normals: (nrm [cap,3], normal_marched [N,3]) - the marching kernel composites the unit SDF gradients as well.
        side_by_side (the train step's default path): geometry forward and colour lookup share one launch unless a
        before_k0_use hook has to run between them.
        composite=False (the train step's default path): the pass stops in front of the compositing - the caller composites, takes
        the ray losses and differentiates the composite in one launch (ops.loss_rays(march=...)) and calls backward(march_done=True)."""
        cfg, sc = self.cfg, self.cfg.pp
        nrm, normal_marched = (None, None) if normals is None else normals
        variant = (not use_deform) or color_thres > 0
        if variant and (side_by_side or before_k0_use is not None or step_w is not None or not composite):
            raise ValueError('use_deform=False / color_thres > 0 are passes of the drop-in module: not inside the fused train step '
                             '(side_by_side, before_k0_use, step_w, composite=False)')
        s = ws                  # whose samples the colour stage and the (second) composite read
        if use_deform:
            ops.warp_fwd(warp_p, ws.pts, ws.count, ws.cap, cfg.out_range, ws.warp_acts, ws.warp_out, self.ctx)
        if variant:
            if use_deform:
                ops.geometry_fwd(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                 ws.alpha, ws.gradient, ws.sdf_final, ws.sdf_deform, ws.grad_deform)
            else:
                ops.geometry_plain_fwd(sc, sdf, sdf_ab, ws.pts, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s, ws.alpha,
                                       ws.gradient, ws.sdf_final)
            if color_thres > 0:
                s = ws.kept_samples()
                ops.alpha2weight_fwd(ws.alpha, ws.ray_start, ws.N, s.weights_all, s.T_all, s.last_all, s.i_end_all)
                ops.keep_compact(s.weights_all, ws.ray_start, ws.N, ws.cap, color_thres, ws.pts, ws.ray_id, ws.step, ws.alpha,
                                 ws.gradient, s.idx, s.ray_start, s.count, s.pts, s.ray_id, s.step, s.alpha, s.gradient)
            ops.color_feat_fwd(sc, k0_cl, s.pts, ws.viewdirs, s.ray_id, s.gradient, pe_w, s.count, ws.cap, ws.feat)
        elif side_by_side and before_k0_use is None and (sc.k0_dim, sc.pos_pe, sc.view_pe) == (12, 5, 1):
            # only the normal columns of feat need the geometry: the colour lookup runs beside it, in the same launch
            ops.geometry_color_feat_fwd(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                        ws.alpha, ws.gradient, ws.sdf_final, ws.sdf_deform, ws.grad_deform, k0_cl, pe_w, ws.feat)
        else:
            ops.geometry_fwd(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                             ws.alpha, ws.gradient, ws.sdf_final, ws.sdf_deform, ws.grad_deform)
            if before_k0_use is not None:
                before_k0_use()             # multi-GPU: the all-gather of the updated grid overlaps everything above
            ops.color_feat_fwd(sc, k0_cl, ws.pts, ws.viewdirs, ws.ray_id, ws.gradient, pe_w, ws.count, ws.cap, ws.feat)
        ops.rgbnet_fwd(rgbnet_p, ws.feat, s.count, ws.cap, ws.rgb_acts, ws.rgb, self.ctx)
        if nrm is not None:
            # rows past the count hold stale values: harmless, the marching kernel walks ray_start ranges only
            torch.div(s.gradient, s.gradient.norm(2, -1, keepdim=True) + 1e-6, out=nrm)
        if not composite:
            if normals is not None or step_w is not None:
                raise ValueError('composite=False: the fused ray launch composites neither normals nor a step_w of the caller')
            return
        ops.march_fwd(s.alpha, ws.rgb, s.step if step_w is None else step_w, nrm, s.ray_start, ws.N, cfg.bg,
                      ws.weights, ws.T, ws.alphainv_last, ws.i_end, ws.rgb_marched, ws.rgb_pre, ws.cum_weights,
                      ws.depth_acc, normal_marched)

    # -- backward ------------------------------------------------------------------------------------------
    def backward(self, ws, k0_cl, sdf, sdf_ab, rgbnet_p, warp_p, inv_s, pe_w, k0_grad_cl, sdf_ab_grad, rgbnet_grad,
                 warp_grad, g_depth=None, g_weights=None, g_gradient_ext=None, g_sdf_deform=None, g_grad_deform=None,
                 g_correction=None, g_alpha_ext=None, g_rgb_ext=None, after_k0_grad=None, priors=None, march_done=False,
                 use_deform=True, color_thres=0.0):
        """Consumes ws.g_rgbm / ws.g_last / ws.g_cw (+ optional per-sample upstream grads), accumulates parameter
        grads (atomic +=) and leaves d/d ray_pts in ws.g_pts and the per-sample viewdir grads in ws.g_view_s.
        march_done: the caller ran ops.loss_rays(march=...) after forward(composite=False) - ws.g_alpha / ws.g_rgb are in place.
        use_deform / color_thres: as handed to forward().  color_thres > 0: g_weights, g_alpha_ext, g_rgb_ext and what
        g_gradient_ext adds are gradients of the KEPT samples (g_gradient_ext receives ws.kept); the composite and the colour stage
        are differentiated there, ops.keep_scatter_bwd carries their sample gradients to the original rows (exact zeros on the
        dropped ones) and the geometry backward runs over every sample.  The first composite carries no gradient: it only decides
        the mask.  use_deform=False: neither warp_grad nor ws.g_warp_out is touched."""
        cfg, sc = self.cfg, self.cfg.pp
        variant = (not use_deform) or color_thres > 0
        if variant and (priors is not None or march_done or after_k0_grad is not None):
            raise ValueError('use_deform=False / color_thres > 0 are passes of the drop-in module: not inside the fused train step '
                             '(priors, march_done, after_k0_grad)')
        s = ws.kept_samples(backward=True) if color_thres > 0 else ws
        if march_done:
            if not (g_depth is None and g_weights is None and g_alpha_ext is None and g_rgb_ext is None):
                raise ValueError('march_done: the fused ray launch takes no upstream gradients beside the ray losses')
        else:
            ops.march_bwd(s.alpha, ws.rgb, s.step, ws.weights, ws.T, ws.alphainv_last, s.ray_start, ws.i_end, ws.N, cfg.bg,
                          ws.rgb_pre, ws.g_rgbm, ws.g_cw, ws.g_last, g_depth, g_weights, s.g_alpha, ws.g_rgb)
        if g_alpha_ext is not None:
            s.g_alpha.add_(g_alpha_ext)
        if g_rgb_ext is not None:
            ws.g_rgb.add_(g_rgb_ext)
        ctx = self.ctx
        ops.rgbnet_bwd(rgbnet_p, ws.feat, ws.rgb_acts, ws.rgb, ws.g_rgb, s.count, ws.cap, ws.scratch_rgb,
                       rgbnet_grad, ws.g_feat, ctx)
        ops.color_feat_bwd(sc, k0_cl, s.pts, ws.viewdirs, s.ray_id, s.gradient, pe_w, s.count, ws.cap, ws.g_feat,
                           k0_grad_cl, s.g_pts, s.g_gradient, s.g_view_s)
        if after_k0_grad is not None:
            after_k0_grad()             # multi-GPU: the grid reduce-scatter overlaps the rest of the backward
        if priors is not None:
            # fused step: the sample-level priors (eikonal, deformation) are differentiated inside the geometry backward
            w_eik, w_dyn, ls, loss_out, batch_norm = priors
            if self.ordered:
                ops.geometry_bwd_priors_ordered(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap,
                                                inv_s, ws.g_alpha, ws.g_gradient, w_eik, w_dyn, ls, 1, ws.g_warp_out, ws.g_pts,
                                                ws.g_view_s, sdf_ab_grad, loss_out, batch_norm, self.ctx)
            else:
                ops.geometry_bwd_priors(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                        ws.g_alpha, ws.g_gradient, w_eik, w_dyn, ls, 1, ws.g_warp_out, ws.g_pts, ws.g_view_s,
                                        sdf_ab_grad, loss_out, batch_norm)
        else:
            if self.ordered:
                raise ValueError('an ordered RenderCore differentiates the fused step only (priors=...): the separate '
                                 'geometry backward keeps its float atomics')
            if g_gradient_ext is not None:
                g_gradient_ext(s)       # callable adding loss terms into g_gradient etc. (of the kept samples when color_thres > 0)
            if s is not ws:
                ops.keep_scatter_bwd(s.idx, s.count, ws.cap, s.g_alpha, s.g_gradient, s.g_pts, s.g_view_s, ws.g_alpha,
                                     ws.g_gradient, ws.g_pts, ws.g_view_s)
            if use_deform:
                ops.geometry_bwd(sc, sdf, sdf_ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                 ws.g_alpha, ws.g_gradient, None, g_sdf_deform, g_grad_deform, g_correction, 1, ws.g_warp_out,
                                 ws.g_pts, ws.g_view_s, sdf_ab_grad)
            else:
                ops.geometry_plain_bwd(sc, sdf, sdf_ab, ws.pts, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s, ws.g_alpha,
                                       ws.g_gradient, None, 1, ws.g_pts, ws.g_view_s, sdf_ab_grad)
        if use_deform:
            ops.warp_bwd(warp_p, ws.pts, ws.warp_acts, ws.g_warp_out, ws.count, ws.cap, cfg.out_range, ws.scratch, warp_grad,
                         ws.g_pts, ctx)


class TrainEngine:
    """Fused object-branch train step on one GPU (rank-local shard of the rays when world_size > 1)."""

    LR = {'k0': 1e-1, 'rgbnet': 1e-3, 'warp': 1e-3, 'sdf_ab': 1e-2}     # configs/dtu_e2e/scan1.py:87-103

    def __init__(self, cfg: SceneConfig, n_views, H, W, n_rand, device='cuda', lr_pose=1e-3, lr_pose_end=1e-4,
                 pose_iters=1, lrate_decay=10, loss_scale=0.1, weight_main=1.0, weight_tv_k0=0.01, weight_mask=0.1,
                 fix_first=True, capacity=None, x_slab=None, dist_ctx=None, deterministic_scatter=False, options=None,
                 deterministic=False, reproj_rows=0, fuse_head=True, fuse_rays=True, fuse_wgrad=True, featproj_rows=0):
        """fuse_head / fuse_rays (default path only, see `side_by_side`): the step starts with ONE launch (ops.step_begin: pose forward,
        step scalars, zero block, weight pack) / composites, evaluates the ray losses and differentiates the composite in ONE launch
        (ops.march_loss_bwd) - DESIGN 17.  False: the separate launches (A/B runs, tests); also plain attributes of the engine.
        fuse_wgrad (default path only, as the two above): the hidden layers' weight gradients of rgbnet ride in the launch of the warp
        net's (pass_scope(join_wgrad=True)).  False: the two launches.
        reproj_rows: row capacity of the engine-native reprojection pass (`reprojection_grads`); each row is one ray of a second
        Workspace(reproj_rows, reproj_rows * n_samples).  0 (default): no second workspace, nothing changes.
        featproj_rows: row capacity of the surface-projection feature pass (`surface_projection_grads`); each row is one ray of a
        Workspace(featproj_rows, featproj_rows * n_samples) for the differentiable query (about 18 KB per sample) and one ray of a
        forward-only workspace for the reference query (no activations, no gradient buffers: about 0.4 KB per sample), i.e.
        18.4 KB * n_samples per row (160^3 voxels, 186 samples: 3.4 MB per row, the reference's 256 rows: 0.9 GB).  0 (default):
        nothing is allocated, no launch differs.
        deterministic: bit-reproducible train step.  Implies deterministic_scatter and additionally replaces every other
        floating-point sum of the object-branch step that feeds a parameter update and depends on the order in which work-groups
        or lanes finish - the weight and bias gradients of both MLPs, their thin layers, the alpha / beta gradient of the geometry
        backward, the pose gradient of the ray backward - by per-work-group (per-ray) partial sums in a workspace and a reduction
        in a fixed order (ops.ordered_attach; sized by ops.ordered_workspace, allocated at the first step and kept).
        GUARANTEE: for a fixed build, fixed option values, fixed shapes and the same device model, identical inputs (state,
        ray_idx, jitter, global_step sequence) give bit-identical k0, k0_m, k0_v, flat.data, flat.m, flat.v, se3, se3_m, se3_v
        after every step.  It is NOT a promise of equal bits across different mlp_wgs values, builds or chips, and it covers the
        single-GPU object branch only: multi-rank runs (dist) work with such an engine but keep their own reductions, and the
        scene branch / joint step need joint.DualBranchEngine(deterministic=True) on top of it.  The reported scalars (ws.loss_out, ws.tv_out) stay on float atomics:
        they feed no update and may differ in the last bits between runs.
        The engine then always owns a private context (the host's default context's values + `options`).  Only the default,
        split-precision layer-fused MLP kernels have ordered flushes: options mlp_fused = 0, mlp_split without bits 2, 8 and 16
        (e.g. mlp_split = 0) are refused with ValueError.  Off (default): nothing changes - same kernels, same launches.
        deterministic_scatter: the k0 gradient is accumulated per voxel in sample order (sorted scatter, ~0.2 ms instead of
        0.04 ms per step) instead of by float atomics - bit-identical gradient grids for identical inputs, and bit-identical
        replicas in the multi-GPU "samples" mode without the periodic re-broadcast.
        options: {name: value} of a PRIVATE pp_context for this engine's kernels (e.g. {'mlp_split': 0}: every MLP product on the
        fp32 MFMA instructions); None = the host's default context.  Engines with different options coexist in one process."""
        self.cfg, self.dev = cfg, torch.device(device)
        self.deterministic = bool(deterministic)
        if self.deterministic:
            from . import _lib
            opts = dict(_lib.default_context().options(), **(options or {}))
            refused = [('mlp_fused = 0: the layer-by-layer kernels', opts['mlp_fused'] != 1),
                       (f"mlp_split = {opts['mlp_split']} (bits 2, 8 and 16 are needed): the fp32-instruction kernels",
                        opts['mlp_split'] & 26 != 26)]
            for what, bad in refused:
                if bad:
                    raise ValueError(f'deterministic=True with {what} have no ordered gradient flush (they keep float atomics)')
            options = opts
            deterministic_scatter = True
        self.ctx = ops.Context(**options) if options else None
        self.deterministic_scatter = bool(deterministic_scatter)
        self._scatter_work = None
        self._ordered_work = None
        self.V, self.H, self.W, self.N = n_views, H, W, n_rand
        cap = capacity or n_rand * cfg.n_samples
        self.ws = Workspace(n_rand, cap, self.dev, ctx=self.ctx)
        self.core = RenderCore(cfg, ctx=self.ctx, ordered=self.deterministic)
        X, Y, Z = cfg.world_size
        f = dict(dtype=torch.float32, device=self.dev)
        self.k0 = [torch.zeros(X, Y, Z, cfg.k0_dim, **f), torch.zeros(X, Y, Z, cfg.k0_dim, **f)]   # ping-pong
        self.k0_cur = 0
        self.k0_grad, self.k0_m, self.k0_v = (torch.zeros(X, Y, Z, cfg.k0_dim, **f) for _ in range(3))
        self.sdf = torch.zeros(X, Y, Z, **f)
        # one byte per voxel, two parities: the scatter of step n marks [n & 1], the fused optimiser pass reads it (voxels that
        # were not reached keep a known-zero gradient: no read, no re-zeroing) and clears the other one for step n+1
        self.k0_touched = torch.zeros(2, X * Y * Z, dtype=torch.uint8, device=self.dev)
        self.touch_par = 0
        self._k0_marked = False
        self.flat = FlatParams(self.dev)
        # weight pack of the two MLPs: written when a pass opens its scope (RenderCore.pass_scope), valid until the scope closes
        self.mlp_pack = torch.empty(ops.mlp_pack_workspace(), **f)
        self.se3 = torch.zeros(n_views, 6, **f)
        self.se3_grad, self.se3_m, self.se3_v = (torch.zeros(n_views, 6, **f) for _ in range(3))
        self.w2c_init = torch.zeros(n_views, 3, 4, **f)
        self.w2c, self.c2w = torch.zeros(n_views, 3, 4, **f), torch.zeros(n_views, 3, 4, **f)
        self.jac = torch.zeros(n_views, 12, 6, **f)
        self.c2w_grad = torch.zeros(n_views, 3, 4, **f)
        # train step on the default path: the optimiser launch carries the ray / pose backward (ops._tail_args).  Its last ray
        # work-group leaves c2w_grad and this arrival counter zero again; _c2w_clean = both are zero now
        self.tail_arrive = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.fuse_head, self.fuse_rays, self.fuse_wgrad = bool(fuse_head), bool(fuse_rays), bool(fuse_wgrad)
        # partial loss rows + arrival ticket of the fused ray launch; None: a ray may have more samples than that kernel holds -
        # the step then keeps march_fwd / loss_rays / march_bwd
        self.ray_work = None
        if cfg.n_samples <= ops.MARCH_LOSS_MAX_SAMPLES:
            self.ray_work = torch.zeros(ops.march_loss_workspace(n_rand, cfg.n_samples), dtype=torch.uint8, device=self.dev)
        elif self.fuse_rays:
            warnings.warn(f'{cfg.n_samples} samples per ray: more than the fused ray launch holds ({ops.MARCH_LOSS_MAX_SAMPLES}); '
                          'the step composites, takes the ray losses and differentiates in separate launches')
        self._c2w_clean = True
        self._deferred_rays = None
        mask = torch.ones(n_views, dtype=torch.int32)
        if fix_first:
            mask[0] = 0                     # get_current_pose_pnp never refines view 0 (recon_scene.py:68)
        self.refine_mask = mask.to(self.dev)
        self.intr = torch.zeros(n_views, 4, **f)
        self.images = self.masks = None
        self.lr = dict(self.LR)
        self.lr_pose = lr_pose
        self.pose_gamma = (lr_pose_end / (1e-10 + lr_pose)) ** (1. / pose_iters)
        self.decay = 0.1 ** (1 / (lrate_decay * 1000))
        self.loss_scale, self.w_main, self.w_tv, self.w_mask = loss_scale, weight_main, weight_tv_k0, weight_mask
        self.n_step = 0
        self.x_slab = x_slab or (0, X)
        self.dist = dist_ctx
        segs = [self.flat.off[n][0] + _pad(self.flat.off[n][1]) for n, _ in FlatParams.SEG]
        self.seg_end = torch.tensor(segs, dtype=torch.int32, device=self.dev)
        self.pose_seg_end = torch.tensor([n_views * 6], dtype=torch.int32, device=self.dev)
        # per-step scalars travel in ONE async H2D copy from a pinned staging buffer:
        #   [0:npe) BARF weights | [npe:npe+3) lr of sdf_ab, rgbnet, warp | [npe+3] pose lr
        self.npe = cfg.posbase_pe + cfg.viewbase_pe
        # ring of pinned slots: the host may run many steps ahead of the GPU (no sync in the step), a slot must not be
        # rewritten before its async copy has executed; the launch queue never holds 256 steps
        self.step_host = torch.zeros(256, self.npe + 4, dtype=torch.float32)
        if self.dev.type == 'cuda':
            self.step_host = self.step_host.pin_memory()
        self._slot = 0
        self.step_dev = torch.zeros(self.npe + 4, **f)
        if self.npe + 4 > ops.STEP_SCALARS_MAX and self.fuse_head:
            # more step scalars than ops.step_begin hands over by value: pose_fwd, the pinned upload and mlp_pack stay separate
            warnings.warn(f'{self.npe} position-encoding bands: the step keeps its separate head launches')
            self.fuse_head = False
        self.pe_w = self.step_dev[:self.npe]
        self.seg_lr = self.step_dev[self.npe:self.npe + 3]
        self.pose_seg_lr = self.step_dev[self.npe + 3:self.npe + 4]
        self.reproj_rows = int(reproj_rows)
        self.ws_reproj = None
        self.last_reproj_terms = None
        if self.reproj_rows > 0:
            self._alloc_reproj()
        self.featproj_rows = int(featproj_rows)
        self.ws_featproj = self.ws_featproj_ref = None
        self.feature_maps = None
        self.last_featproj_terms = None
        if self.featproj_rows > 0:
            self._alloc_featproj()

    def _alloc_aux(self, R):
        """What each auxiliary pass (reprojection_grads, surface_projection_grads) owns: a workspace of its own for R rays (the main
        pass's activations stay untouched) whose ray-level colour gradients are zero for good - the passes have depth-only losses -,
        and the per-row and per-view gradient buffers of their common backward (_depth_loss_pass, _pose_fold)."""
        ws = Workspace(R, R * self.cfg.n_samples, self.dev, ctx=self.ctx)
        for t in (ws.g_rgbm, ws.g_last, ws.g_cw):
            t.zero_()
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.dev)
        return ws, dict(g_depth=z(R), g_o=z(R, 3), g_d=z(R, 3), go=z(R, 3), gd=z(R, 3), gv=z(R, 3), g_w2c=z(self.V, 3, 4),
                        g_c2w=z(self.V, 3, 4), se3=z(self.V, 6))

    def _alloc_reproj(self):
        """Buffers of reprojection_grads: _alloc_aux and what pp_reproj_loss and the crossing query write per row."""
        R, cfg = self.reproj_rows, self.cfg
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.dev)
        self.ws_reproj, self._rp = self._alloc_aux(R)
        self._rp.update(g_p=z(R, 3), g_t=z(R), p=z(R, 3), hit=torch.zeros(R, dtype=torch.uint8, device=self.dev), terms=z(3))
        # the reference's "centre" and diagonal (lib/recon_scene.py:344, lib/voxurf_coarse.py:102; both sic), in its fp32 arithmetic
        lo, hi = (torch.tensor(np.asarray(a, dtype=np.float32)) for a in (cfg.xyz_min, cfg.xyz_max))
        self._rp_centre = [float(x) for x in (lo + hi)]
        self._rp_half_diag = float(torch.sqrt(torch.sum(hi - lo ** 2)) / 2.)        # = Voxurf.diagonal_length / 2 (voxurf_coarse.py)
        if not math.isfinite(self._rp_half_diag):
            # the (sic) formula has a negative radicand for such a box: torch.clamp then propagates NaN, the kernel's fmaxf would not
            raise ValueError('reproj_rows > 0: Voxurf.diagonal_length is not finite for this box (sum(xyz_max - xyz_min ** 2) < 0)')

    def _alloc_featproj(self):
        """Buffers of surface_projection_grads: _alloc_aux for query A, a forward-only workspace for query B, and the per-row buffers
        of the pp_featproj_* kernels."""
        R = self.featproj_rows
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.dev)
        self.ws_featproj, self._fp = self._alloc_aux(R)
        self.ws_featproj_ref = Workspace(R, R * self.cfg.n_samples, self.dev, backward=False, keep_activations=False, ctx=self.ctx)
        self._fp.update(own_ref=torch.zeros(R, dtype=torch.int32, device=self.dev), pix_ref=z(R, 2), terms=z(2 + ops.FEATPROJ_MAX_LAYERS),
                        valid=torch.zeros(R, dtype=torch.uint8, device=self.dev), cos=z(ops.FEATPROJ_MAX_LAYERS, R), g_q=z(R, 6))

    # ---- data / parameter loading ---------------------------------------------------------------------------
    def set_feature_maps(self, features):
        """features: 1 to 4 per-view feature maps [V, C, h, w] (the reference's data_dict['vgg_features']; any tensors of that
        shape, numpy or torch), 1 <= C <= 512, h, w >= 2.  Converted ONCE to the layout the gather reads - channels-last [V, h, w, C]
        fp32 on the device - and kept."""
        maps = []
        for t in features:
            t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t)
            if t.dim() != 4 or t.shape[0] != self.V:
                raise ValueError(f'a feature map must be [n_views = {self.V}, C, h, w], got {tuple(t.shape)}')
            if not (1 <= t.shape[1] <= ops.FEATPROJ_MAX_CHANNELS and t.shape[2] >= 2 and t.shape[3] >= 2):
                raise ValueError(f'a feature map needs 1 <= C <= {ops.FEATPROJ_MAX_CHANNELS} and h, w >= 2, got {tuple(t.shape)}')
            maps.append(t.detach().to(self.dev, torch.float32).permute(0, 2, 3, 1).contiguous())
        if not 1 <= len(maps) <= ops.FEATPROJ_MAX_LAYERS:
            raise ValueError(f'{len(maps)} feature maps: need 1 to {ops.FEATPROJ_MAX_LAYERS}')
        self.feature_maps = maps

    def set_views(self, images, masks, Ks, w2c_init):
        """images [V,H,W,3], masks [V,H,W,1|none], Ks [V,3,3], w2c_init [V,3,4] (numpy or torch)."""
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.dev).contiguous()
        self.images, self.masks = t(images), t(masks).reshape(self.V, self.H, self.W).contiguous()
        K = torch.as_tensor(np.asarray(Ks), dtype=torch.float32)
        self.intr.copy_(torch.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], -1))
        self.w2c_init.copy_(t(w2c_init))

    @property
    def k0_cl(self):
        return self.k0[self.k0_cur]

    def load_reference_params(self, k0, sdf, sdf_alpha, sdf_beta, rgbnet, warp, se3=None):
        """k0 [1,C,X,Y,Z], sdf [1,1,X,Y,Z] in the reference layout (state_dict tensors)."""
        with torch.no_grad():
            self.k0_cl.copy_(k0[0].permute(1, 2, 3, 0).to(self.dev))
            self.sdf.copy_(sdf[0, 0].to(self.dev))
            d = lambda x: x.detach().to(self.dev)
            self.flat.load_reference(d(sdf_alpha), d(sdf_beta), [(d(W), d(b)) for W, b in rgbnet],
                                     [(d(W), d(b)) for W, b in warp])
            if se3 is not None:
                self.se3.copy_(se3.to(self.dev))

    def set_template(self, sdf):
        """Install a frozen SDF template: sdf [X,Y,Z] or [1,1,X,Y,Z] (negative inside; tensor or numpy, any device), copied into the
        engine's `sdf` as load_reference_params copies its own.  mesh.signed_distance_grid makes one from a mesh."""
        sdf = torch.as_tensor(sdf)
        if sdf.dim() == 5 and tuple(sdf.shape[:2]) == (1, 1):
            sdf = sdf[0, 0]
        if tuple(sdf.shape) != tuple(self.sdf.shape):
            raise ValueError(f'set_template: the template is {tuple(sdf.shape)}, the engine\'s grid {tuple(self.sdf.shape)}')
        with torch.no_grad():
            self.sdf.copy_(sdf.detach().to(self.dev))

    def k0_reference_layout(self, t=None):
        t = self.k0_cl if t is None else t
        return t.permute(3, 0, 1, 2)[None]

    # ---- one step -------------------------------------------------------------------------------------------
    def scatter_work(self, n_samples):
        """Workspace of the deterministic scatter (grown on demand, kept)."""
        need = ops.k0_scatter_sorted_workspace(n_samples)
        if self._scatter_work is None or self._scatter_work.numel() < need:
            self._scatter_work = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._scatter_work

    def ordered_work(self):
        """Workspace of the ordered gradient flushes (deterministic=True): allocated on first use for this engine's shapes, attached
        to its context and kept."""
        mlp_wgs = self.ctx.get('mlp_wgs')
        wgs = max(16, mlp_wgs) if mlp_wgs > 0 else torch.cuda.get_device_properties(self.dev).multi_processor_count
        need = ops.ordered_workspace(wgs, self.ws.cap, self.N)
        if self._ordered_work is None or self._ordered_work.numel() < need:
            self._ordered_work = torch.empty(need, dtype=torch.uint8, device=self.dev)
            ops.ordered_attach(self.ctx, self._ordered_work, wgs, self.ws.cap, self.N)
        return self._ordered_work

    def zero_grads(self):
        self.k0_grad.zero_()
        self.k0_touched.zero_()
        self._k0_marked = False
        self.flat.grad.zero_()
        self.se3_grad.zero_()
        self.c2w_grad.zero_()
        self.tail_arrive.zero_()
        self._c2w_clean = True
        self._deferred_rays = None

    @property
    def side_by_side(self):
        """The default path (single GPU, no ordered flush): independent small kernels ride in a neighbour's launch."""
        return self.dist is None and not self.deterministic

    def render_and_grads(self, ray_idx, jitter, global_step, defer_pose_bwd=False):
        """pose -> rays -> forward -> losses -> full backward.  Gradients are accumulated into k0_grad / flat.grad /
        se3_grad (which must be zero on entry).
        defer_pose_bwd (train_step only; default path only): the ray / pose backward is left to the optimiser launch of THIS step -
        se3_grad is not complete when this returns, optimizer_step must follow before anything reads it."""
        defer_pose_bwd = defer_pose_bwd and self.side_by_side
        self._deferred_rays = None
        cfg, ws, sc = self.cfg, self.ws, self.cfg.pp
        if self.deterministic:
            self.ordered_work()
        progress = global_step / cfg.N_iters
        P = self.flat
        head = None
        if self.side_by_side and self.fuse_head:
            # one launch for everything the step needs before its first ray.  The pack is made HERE, at the start of the
            # step that uses it, so a parameter write between two steps (checkpoint load, in-place copy) is seen
            head = lambda: ops.step_begin(self.se3, self.w2c_init, self.refine_mask, self.w2c, self.c2w, self.jac,
                                          self._step_scalars(progress), self.step_dev, ws.zero_block, P.view('warp'),
                                          P.view('rgbnet'), self.mlp_pack, self.ctx)
        fused_rays = self.side_by_side and self.fuse_rays and self.ray_work is not None
        s_val, inv_s = cfg.s_val(global_step), cfg.inv_s(global_step)
        w_dyn = dynamic_weight(1e-1, 1e-3, global_step, cfg.N_iters)
        ls = self.loss_scale

        def rays_and_samples():
            ops.raygen_select_fwd(sc, ray_idx, self.c2w, self.intr, self.H, self.W, cfg.inverse_y, True, self.images, self.masks,
                                  ws.rays_o, ws.rays_d, ws.viewdirs, ws.target, ws.mask_px)
            self.core.sample(ws, jitter)
            if self.dist is not None:
                # (sample count, masked-pixel count) of every rank: sizes the sample exchange exactly and normalises the losses
                # over the union batch; the 8-byte all-gather completes under the forward pass
                self.dist.start_batch_stats(ws.count, ws.mask_px)
        if head is None:
            # separate launches, in the order they always had: pose, rays, samples, scalars; the scope then packs
            ops.pose_fwd(self.se3, self.w2c_init, self.refine_mask, self.w2c, self.c2w, self.jac)
            rays_and_samples()
            self._upload_step_scalars(progress)
        with self.core.pass_scope(P, self.mlp_pack, ws, pack_with=head, join_wgrad=self.side_by_side and self.fuse_wgrad):
            if head is not None:
                rays_and_samples()          # behind the head launch, which the scope has just issued
            self.core.forward(ws, self.k0_cl, self.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), inv_s, self.pe_w,
                              before_k0_use=None if self.dist is None else (lambda: self.dist.wait_parameters(self)),
                              side_by_side=self.side_by_side, composite=not fused_rays)
            if head is None:
                ws.zero_block.zero_()
            batch_norm = None if self.dist is None else self.dist.wait_batch_stats()
            # fused_rays: the composite, the ray losses and the compositing backward of a ray by one wavefront, in this launch
            march = (ws.alpha, ws.rgb, ws.step, ws.ray_start, cfg.n_samples, cfg.bg, ws.weights, ws.T, ws.i_end, ws.rgb_pre,
                     ws.depth_acc, ws.g_alpha, ws.g_rgb, self.ray_work) if fused_rays else None
            ops.loss_rays(ws.rgb_marched, ws.alphainv_last, ws.cum_weights, ws.target, ws.mask_px, ws.mask_sum, self.w_main,
                          0.01, self.w_mask, ls, ws.g_rgbm, ws.g_last, ws.g_cw, ws.loss_out, batch_norm, march=march)

            # The k0 scatter is issued from here (not inside colour-feature backward) so that it can mark the voxels it reaches:
            # single GPU = right after the colour-feature backward; multi-GPU "samples" mode = replayed for all ranks' gathered
            # samples at the end of the backward; "zero1" = dense reduce-scatter, no marking (every voxel may be non-zero).
            dense_exchange = self.dist is not None and self.dist.local_scatter
            k0_grad = self.k0_grad if dense_exchange else None
            self._k0_marked = not dense_exchange
            touched = self.k0_touched[self.touch_par]

            def after_k0():
                if self.dist is None:
                    if self.deterministic_scatter:
                        ops.k0_scatter_samples_sorted(sc, ws.pts, ws.count, ws.cap, ws.g_feat, self.k0_grad, self.scatter_work(ws.cap), touched)
                    else:
                        ops.k0_scatter_samples(sc, ws.pts, ws.count, ws.cap, ws.g_feat, self.k0_grad, touched)
                else:
                    self.dist.start_grid_reduce(self)
            self.core.backward(ws, self.k0_cl, self.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), inv_s, self.pe_w,
                               k0_grad, P.view('sdf_ab', 'grad'), P.view('rgbnet', 'grad'), P.view('warp', 'grad'),
                               priors=(1.0, w_dyn, ls, ws.loss_out, batch_norm),
                               after_k0_grad=after_k0, march_done=fused_rays)
            if defer_pose_bwd:
                self._deferred_rays = ray_idx
            elif self.deterministic:
                ops.raygen_select_bwd_ordered(sc, ray_idx, self.c2w, self.intr, self.H, self.W, cfg.inverse_y, ws.rays_o, ws.rays_d,
                                              ws.t_min, ws.ray_start, ws.g_pts, ws.step, ws.g_view_s, None, None, None, None, None,
                                              None, None, self.c2w_grad, self.ctx)
            else:
                ops.raygen_select_bwd(sc, ray_idx, self.c2w, self.intr, self.H, self.W, cfg.inverse_y, ws.rays_o, ws.rays_d,
                                      ws.t_min, ws.ray_start, ws.g_pts, ws.step, ws.g_view_s, None, None, None, None, None, None,
                                      None, self.c2w_grad)
            if not defer_pose_bwd:
                self._c2w_clean = False
                ops.pose_bwd(self.jac, self.c2w_grad, self.se3_grad)
        return s_val, w_dyn

    # ---- the auxiliary passes: a second ray batch through the object branch's kernels, on buffers of its own (_alloc_aux) ----------
    def _refuse_aux(self, name, ws, method, capacity):
        """What neither auxiliary pass does.  name: the pass in the messages' words; ws: its workspace, None without `capacity`."""
        if ws is None:
            raise ValueError(f'{method} needs an engine built with {capacity} > 0')
        if self.deterministic:
            raise ValueError(f'the {name} pass is out of the scope of deterministic=True: its render backward uses the separate '
                             'geometry backward, which keeps float atomics')
        if self.dist is not None:
            raise NotImplementedError(f'the {name} pass is not sharded across ranks')
        if not self.cfg.inverse_y:
            raise NotImplementedError(f'the {name} pass implements inverse_y=True without flips (the DTU setting)')

    def _row_jitter(self, jitter, cap):
        """Training-mode per-ray jitter over a pass's whole capacity.  None: drawn on the device; shorter: zero-padded (the rows past
        the caller's are rays that miss the box: any jitter will do)."""
        if jitter is None:
            return torch.rand(cap, device=self.dev)
        return jitter if jitter.shape[0] >= cap else torch.cat([jitter, jitter.new_zeros(cap - jitter.shape[0])])

    def _depth_loss_pass(self, ws, b, view, pix, n, global_step, loss):
        """The sampled rays of `ws` rendered and differentiated for a loss on their depth, then folded into the pose: a weight pack and
        a lean scope of the pass's own, on its own buffers (render_and_grads closed its ones); forward; loss(par) - it leaves the
        loss's gradients in b['g_depth'] (depth), b['g_o'] / b['g_d'] (ray, direct) and b['g_w2c'] -; backward; ray backward; _pose_fold."""
        P = self.flat
        par = (self.k0_cl, self.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), self.cfg.inv_s(global_step), self.pe_w)
        with self.core.pass_scope(P, self.mlp_pack, ws):
            self.core.forward(ws, *par)
            loss(par)
            # depth-only loss: ws.g_rgbm / g_last / g_cw stay zero; no colour-grid gradient is requested (k0_grad = None, no scatter)
            self.core.backward(ws, *par, None, P.view('sdf_ab', 'grad'), P.view('rgbnet', 'grad'), P.view('warp', 'grad'),
                               g_depth=b['g_depth'])
            ops.raygen_select_bwd(self.cfg.pp, None, None, None, 0, 0, True, ws.rays_o, ws.rays_d, ws.t_min, ws.ray_start, ws.g_pts,
                                  ws.step, ws.g_view_s, b['g_o'], b['g_d'], None, b['g_depth'], b['go'], b['gd'], b['gv'], None)
        self._pose_fold(ws, b, view, pix, n, b['gv'], None)

    def _pose_fold(self, ws, b, view, pix, n, g_v, g_t):
        """Ray gradients b['go'] / b['gd'] (+ g_v on viewdirs, g_t on t_min; None: none) of the rows' views and the loss's direct
        b['g_w2c'] -> c2w -> through the step's Jacobian, ADDED to se3_grad."""
        ops.reproj_pose_fold(self.cfg.pp, view, pix, n, self.intr, self.c2w, self.w2c, ws.rays_o, ws.rays_d, b['go'], b['gd'], g_v, g_t,
                             b['g_w2c'], b['g_c2w'])
        ops.pose_bwd(self.jac, b['g_c2w'], b['se3'])
        self.se3_grad += b['se3']

    def reprojection_grads(self, rows, mode, global_step, jitter=None, weight_projection=1.0, weight_near_surface=1.0, nl=0.0,
                           pixel_thre=None, scale=None):
        """Reprojection + near-surface terms of matched pixels (recon_utils.get_project_error; lib/recon_scene.py:321-369, :621-637)
        inside the engine's own launches: the rows become a second ray batch that goes through the object branch's kernels on a
        workspace of its own, and the gradient of scale * (weight_near_surface * near + weight_projection * err) is ACCUMULATED
        into flat.grad (warp network, sdf_alpha / sdf_beta; mode 'render' only) and se3_grad.  k0_grad / k0_touched are left
        exactly as they are.  No autograd, no host synchronisation, no parameter copy.
        Must run after render_and_grads and before optimizer_step: it uses that step's w2c / c2w / jac and BARF weights.
        rows: dict(own, other [R] int32 view indices, pix [R,2] pixel (x, y) in the own view, match [R,2] matched pixel in the
        other view, conf [R]; optional n_rows <= R: the rows in play), R <= reproj_rows.
        mode: 'crossing' - surface point = first zero crossing of the raw template (query_sdf_point_wocuda_wodeform; the reference
        while at most two views are active) - or 'render' - expected ray depth of the full render
        (query_sdf_point_wocuda_render).  jitter [R] (training-mode per-ray jitter); None: drawn on the device.
        scale: None = the engine's loss_scale.  Leaves last_reproj_terms = dict(err, near, n_valid) as device tensors."""
        self._refuse_aux('reprojection', self.ws_reproj, 'reprojection_grads', 'reproj_rows')
        if mode not in ('crossing', 'render'):
            raise ValueError(f"mode must be 'crossing' or 'render', got {mode!r}")
        cfg, ws, sc, rp, cap = self.cfg, self.ws_reproj, self.cfg.pp, self._rp, self.reproj_rows
        R = rows['own'].shape[0]
        n = int(rows.get('n_rows', R))
        if not 0 < n <= R <= cap:
            raise ValueError(f'{n} of {R} rows with reproj_rows = {cap}')
        jitter = self._row_jitter(jitter, cap)
        scale = self.loss_scale if scale is None else scale
        ops.reproj_rays(sc, rows['own'], rows['pix'], n, self.intr, self.c2w, ws.rays_o, ws.rays_d, ws.viewdirs)
        self.core.sample(ws, jitter)
        loss_args = (self.intr, self.w2c, self._rp_centre, self._rp_half_diag, nl, pixel_thre, weight_near_surface,
                     weight_projection, scale, rp['terms'], rp['g_p'], rp['g_depth'], rp['g_o'], rp['g_d'], rp['g_w2c'])
        if mode == 'render':
            self._depth_loss_pass(ws, rp, rows['own'], rows['pix'], n, global_step, lambda par: ops.reproj_loss(
                True, n, rows['other'], rows['match'], rows['conf'], ws.rays_o, ws.rays_d, None, None, ws.t_min, ws.depth_acc, *loss_args))
        else:
            S = cfg.n_samples
            dist = cfg.step_dist
            dense, sdf_d = ws.alpha, ws.sdf_final                   # [cap * S] each: free in this mode
            ops.reproj_dense_pts(sc, ws.rays_o, ws.rays_d, ws.t_min, jitter, ws.pts)
            ops.grid_sample_fwd(sc, self.sdf, 1, ws.pts, 1, dense)
            ops.sdf_first_crossing(dense, None, None, cap, S, dist, ws.t_min, ws.rays_o, ws.rays_d, sdf_d, rp['p'], rp['hit'], None)
            ops.reproj_loss(False, n, rows['other'], rows['match'], rows['conf'], ws.rays_o, ws.rays_d, rp['p'], rp['hit'], None,
                            None, *loss_args)
            ops.sdf_crossing_dense_bwd(sc, self.sdf, ws.rays_o, ws.rays_d, ws.t_min, jitter, cap, S, dist, sdf_d, rp['g_p'], None,
                                       rp['go'], rp['gd'], rp['g_t'])
            rp['go'].add_(rp['g_o'])
            rp['gd'].add_(rp['g_d'])
            self._pose_fold(ws, rp, rows['own'], rows['pix'], n, None, rp['g_t'])
        t = rp['terms']
        self.last_reproj_terms = dict(err=t[0], near=t[1], n_valid=t[2])
        return self.last_reproj_terms

    def surface_projection_grads(self, rows, global_step, weight, nl, jitter=None, jitter_ref=None, scale=None):
        """Surface-projection feature loss of one view pair (recon_utils.get_project_feature_loss; lib/recon_scene.py:371-439,
        :610-619) inside the engine's own launches: the rows are a second ray batch through the object branch's kernels on a
        workspace of its own (query A), their surface points are projected into view `other`, a forward-only third batch (query B)
        renders there and decides which rows see the same surface, and the cosine distance of the feature maps (set_feature_maps)
        at the two projections is differentiated by the pp_featproj_* kernels.  The gradient of scale * weight * L is ACCUMULATED
        into flat.grad (warp network, sdf_alpha / sdf_beta) and se3_grad (views own, other and the rows' source views).  k0_grad /
        k0_touched are left exactly as they are.  No autograd, no host synchronisation, no parameter copy.
        Must run after render_and_grads and before optimizer_step: it uses that step's w2c / c2w / jac and BARF weights.
        rows: dict(src [R] int32 source view of each ray, pix [R,2] pixel (x, y) it goes through - pixel centres are x + 0.5,
        y + 0.5 -, own = i, other = j the view pair; optional n_rows <= R: the rows in play), R <= featproj_rows.
        jitter / jitter_ref [R]: the training-mode per-ray jitter of query A / B; None: drawn on the device.  nl > 0: near plane.
        scale: None = the engine's loss_scale.  Leaves last_featproj_terms = dict(loss, n_valid, cos [n_layers]: the per-layer
        sums of cos over the valid rows) as device tensors.  Without a valid row the term and its gradients are exactly 0 (the
        reference: NaN)."""
        self._refuse_aux('surface-projection', self.ws_featproj, 'surface_projection_grads', 'featproj_rows')
        if self.feature_maps is None:
            raise ValueError('surface_projection_grads needs feature maps (set_feature_maps)')
        cfg, ws, wb, sc, fp, cap = self.cfg, self.ws_featproj, self.ws_featproj_ref, self.cfg.pp, self._fp, self.featproj_rows
        R = rows['src'].shape[0]
        n = int(rows.get('n_rows', R))
        if not 0 < n <= R <= cap:
            raise ValueError(f'{n} of {R} rows with featproj_rows = {cap}')
        i, j = int(rows['own']), int(rows['other'])
        if not (0 <= i < self.V and 0 <= j < self.V):
            raise ValueError(f'view pair ({i}, {j}) with {self.V} views')
        jitter, jitter_ref = self._row_jitter(jitter, cap), self._row_jitter(jitter_ref, cap)
        scale = self.loss_scale if scale is None else scale
        ops.reproj_rays(sc, rows['src'], rows['pix'], n, self.intr, self.c2w, ws.rays_o, ws.rays_d, ws.viewdirs)
        self.core.sample(ws, jitter)

        def loss(par):
            # query B: rays of view j through the projections; its forward stores nothing a backward would need
            ops.featproj_reproject(n, j, ws.rays_o, ws.rays_d, ws.t_min, ws.depth_acc, self.intr, self.w2c, nl, fp['own_ref'],
                                   fp['pix_ref'])
            ops.reproj_rays(sc, fp['own_ref'], fp['pix_ref'], n, self.intr, self.c2w, wb.rays_o, wb.rays_d, wb.viewdirs)
            self.core.sample(wb, jitter_ref)
            self.core.forward(wb, *par)
            ops.featproj_loss(n, i, j, ws.rays_o, ws.rays_d, ws.t_min, ws.depth_acc, wb.rays_o, wb.rays_d, wb.t_min, wb.depth_acc,
                              self.intr, self.w2c, nl, cfg.voxel_size, self.H, self.W, self.feature_maps, weight, scale, fp['terms'],
                              fp['valid'], fp['cos'], fp['g_q'], fp['g_depth'], fp['g_o'], fp['g_d'], fp['g_w2c'])
        self._depth_loss_pass(ws, fp, rows['src'], rows['pix'], n, global_step, loss)
        t = fp['terms']
        self.last_featproj_terms = dict(loss=t[0], n_valid=t[1], cos=t[2:2 + len(self.feature_maps)])
        return self.last_featproj_terms

    def _upload_step_scalars(self, progress):
        """BARF weights for this step and the learning rates the optimiser will use at the END of this step (the
        per-step exponential decay precedes the optimiser step, recon_scene.py:742-768)."""
        h = self.step_host[self._slot]
        self._slot = (self._slot + 1) % self.step_host.shape[0]
        h.copy_(torch.from_numpy(self._step_scalars(progress)))
        self.step_dev.copy_(h, non_blocking=True)

    def _step_scalars(self, progress):
        """The npe + 4 floats of step_dev for this step (layout: see step_host), as float32 on the host."""
        d = self.decay
        lrs = np.array([self.lr['sdf_ab'] * d, self.lr['rgbnet'] * d, self.lr['warp'] * d, self.lr_pose], dtype=np.float32)
        return np.concatenate([self.cfg.pe_weights(progress), lrs])

    def optimizer_step(self, optimize_pose=True, grad_scale=1.0):
        cfg = self.cfg
        self.n_step += 1
        for k in self.lr:                       # per-step exponential decay precedes the step (recon_scene.py:742-768)
            self.lr[k] *= self.decay
        if self.side_by_side:
            self._k0_step(self.lr['k0'], self.n_step, grad_scale, tail=self._optimizer_tail(optimize_pose))
            if optimize_pose:
                self.lr_pose *= self.pose_gamma
            return
        self._k0_step(self.lr['k0'], self.n_step, grad_scale)
        if self.dist is not None:
            self.dist.wait_small()          # the small all-reduce (MLP / alpha-beta / pose gradients) ran beside the grid pass
        ops.adam_flat(self.flat.data, self.flat.grad, self.flat.m, self.flat.v, self.seg_end, self.seg_lr, grad_scale, 0.9,
                      0.99, 1e-8, self.n_step, 1)
        if optimize_pose:
            ops.adam_flat(self.se3.view(-1), self.se3_grad.view(-1), self.se3_m.view(-1), self.se3_v.view(-1),
                          self.pose_seg_end, self.pose_seg_lr, grad_scale, 0.9, 0.999, 1e-8, self.n_step, 1)
            self.lr_pose *= self.pose_gamma

    def _optimizer_tail(self, optimize_pose):
        """What the grid pass's launch carries beside it (ops._tail_args): both flat Adam updates and, when render_and_grads left
        it to this launch, the ray / pose backward."""
        ws, cfg, rays = self.ws, self.cfg, None
        if self._deferred_rays is not None:
            if not self._c2w_clean:         # a separate ray backward ran since: its sums are still in c2w_grad
                self.c2w_grad.zero_()
                self.tail_arrive.zero_()
                self._c2w_clean = True
            rays = (cfg.pp, self._deferred_rays, self.c2w, self.intr, self.H, self.W, cfg.inverse_y, ws.rays_o, ws.rays_d, ws.t_min,
                    ws.ray_start, ws.g_pts, ws.step, ws.g_view_s, self.jac, self.c2w_grad, self.tail_arrive)
            self._deferred_rays = None
        pose = None
        if optimize_pose or rays is not None:
            pose = (self.se3.view(-1), self.se3_grad.view(-1), self.se3_m.view(-1), self.se3_v.view(-1), self.pose_seg_lr, 0.9, 0.999,
                    1e-8, optimize_pose)
        return dict(flat=(self.flat.data, self.flat.grad, self.flat.m, self.flat.v, self.seg_end, self.seg_lr, 0.9, 0.99, 1e-8),
                    pose=pose, rays=rays)

    def _k0_step(self, lr_k0, n_step, grad_scale, tail=None):
        """Fused TV + Adam pass over the colour grid (ping-pong buffers flip).  tail: see _optimizer_tail."""
        kw = {} if tail is None else dict(tail=tail)
        cfg = self.cfg
        X, Y, Z = cfg.world_size
        tv_scale = self.loss_scale * self.w_tv / (3.0 * X * Y * Z * cfg.k0_dim)
        src, dst = self.k0[self.k0_cur], self.k0[1 - self.k0_cur]
        xb, xe = self.x_slab
        if self._k0_marked and (xb, xe) == (0, X):
            cur = self.touch_par
            ops.grid_tv_adam_step_sparse(src, dst, self.k0_grad, self.k0_m, self.k0_v, cfg.world_size, cfg.k0_dim, xb, xe,
                                         tv_scale, grad_scale, lr_k0, 0.9, 0.99, 1e-8, n_step, self.ws.tv_out,
                                         self.k0_touched[cur], self.k0_touched[1 - cur], self.ctx, **kw)
            self.touch_par = 1 - cur
            self._k0_marked = False
        else:
            ops.grid_tv_adam_step(src, dst, self.k0_grad, self.k0_m, self.k0_v, cfg.world_size, cfg.k0_dim, xb, xe, tv_scale,
                                  grad_scale, lr_k0, 0.9, 0.99, 1e-8, n_step, self.ws.tv_out, self.ctx, **kw)
        self.k0_cur = 1 - self.k0_cur

    def train_step(self, ray_idx, jitter, global_step, optimize_pose=True):
        """Gradients are zeroed by the optimiser kernels themselves after use; call zero_grads() once before the
        first step."""
        out = self.render_and_grads(ray_idx, jitter, global_step, defer_pose_bwd=True)
        self.grad_scale = 1.0
        if self.dist is not None:
            self.dist.reduce_gradients(self)          # sets x_slab and grad_scale = 1/world
        self.optimizer_step(optimize_pose, grad_scale=self.grad_scale)
        if self.dist is not None:
            self.dist.gather_parameters(self)
        return out

    # ---- checkpoint / resume (wire format of recon_scene.save_checkpoints, lib/recon_scene.py:779-790) -------------
    def _mlp_state(self, which='data'):
        """(state_dict prefix, W, b) of every layer of both MLPs: views into flat.<which> in the reference's logical shapes."""
        for net in ('rgbnet', 'warp'):
            for (*_, key), (W, b) in zip(MLP_LAYOUT[net], _unpack(net, self.flat.view(net, which))):
                yield key, W, b

    def model_state_dict(self):
        """The trainable state under the reference's state_dict names and logical shapes (lib/voxurf_coarse.py module tree,
        SURVEY 8b), so that `Voxurf.load_state_dict(..., strict=False)` of either implementation accepts it."""
        c = lambda t: t.detach().clone().cpu()
        cfg, P = self.cfg, self.flat
        sd = {'sdf_alpha': c(P.view('sdf_ab')[0:1]), 'sdf_beta': c(P.view('sdf_ab')[1:2]),
              'xyz_min': torch.tensor(np.asarray(cfg.xyz_min, dtype=np.float32)),
              'xyz_max': torch.tensor(np.asarray(cfg.xyz_max, dtype=np.float32)),
              'sdf.grid': c(self.sdf)[None, None], 'k0.grid': c(self.k0_reference_layout()).contiguous()}
        for name in ('sdf', 'k0'):
            sd[name + '.xyz_min'], sd[name + '.xyz_max'] = sd['xyz_min'].clone(), sd['xyz_max'].clone()
        for key, W, b in self._mlp_state():
            sd[key + '.weight'], sd[key + '.bias'] = c(W).contiguous(), c(b)
        return sd

    def voxurf_view(self, model=None):
        """The drop-in `Voxurf` module over this engine's CURRENT parameters, for the callers either side of the train step
        that want the module API (surface queries, reprojection losses, inference): built once from `model_kwargs()`; every
        call re-points `k0.grid` at the live ping-pong buffer (zero-copy, channels-last) and the SDF template at the engine's,
        and copies the small parameters (alpha / beta, both MLPs: 370 KB) on the device.  Nothing goes through the host."""
        from . import voxurf_coarse
        if model is None:
            model = voxurf_coarse.Voxurf(**self.model_kwargs()).to(self.dev)
        P = self.flat
        with torch.no_grad():
            model.k0.grid.data = self.k0_reference_layout()
            model.sdf.grid.data = self.sdf[None, None]
            model.sdf_alpha.data.copy_(P.view('sdf_ab')[0:1])
            model.sdf_beta.data.copy_(P.view('sdf_ab')[1:2])
            sd = dict(model.named_parameters())
            for key, W, b in self._mlp_state():
                sd[key + '.weight'].data.copy_(W)
                sd[key + '.bias'].data.copy_(b)
        return model

    def load_model_state_dict(self, sd):
        rg, wp = ([(sd[k + '.weight'], sd[k + '.bias']) for *_, k in MLP_LAYOUT[net]] for net in ('rgbnet', 'warp'))
        self.load_reference_params(sd['k0.grid'], sd['sdf.grid'], sd['sdf_alpha'], sd['sdf_beta'], rg, wp)

    # ---- optimiser state in the reference's layout ---------------------------------------------------------------------
    # lib/recon_scene.py:779-791 stores `self.optimizer.state_dict()` of lib.utils.Adam (a torch.optim.Optimizer): 'state'
    # {param index: {'step', 'exp_avg', 'exp_avg_sq'}} + 'param_groups' [{'name', 'lr', 'params': [indices], ...}], one group
    # per `lrate_<name>` key, parameters in `module.parameters()` order (warp_network starts with its gradient-less
    # `progress`, which never gets a state entry).
    # Group order = the order of the `lrate_<name>` keys of the MERGED training config (lib/utils.py:320-341 walks cfg_train.keys()):
    # configs/default_fine_s.py contributes lrate_k0, lrate_rgbnet (coarse_train :34-35) and lrate_sdf (surf_train :77) first, the keys
    # configs/dtu_e2e/scan1.py:87-103 adds (lrate_sdf_alpha, lrate_sdf_beta, ..., lrate_warp_network) follow in its own order (mmengine
    # merges a child into its base: existing keys keep their place, new ones are appended).  `sdf` (lrate_sdf = 0.1 > 0) IS a group: its
    # one parameter, the frozen template, never receives a gradient, so it holds a parameter index but no state entry.
    GROUPS = ('k0', 'rgbnet', 'sdf', 'sdf_alpha', 'sdf_beta', 'warp_network')

    def _group_tensors(self, which):
        """{group name: list of tensors in the reference's parameter order and logical shapes} for 'm' or 'v'."""
        P = self.flat
        ab = P.view('sdf_ab', which)
        k0 = {'m': self.k0_m, 'v': self.k0_v}[which]
        rg = [t for Wb in unpack_rgbnet(P.view('rgbnet', which)) for t in Wb]
        wp = [t for Wb in unpack_warp(P.view('warp', which)) for t in Wb]
        return {'sdf_alpha': [ab[0:1]], 'sdf_beta': [ab[1:2]], 'k0': [self.k0_reference_layout(k0)], 'rgbnet': rg,
                'sdf': [None],                                     # None = a parameter without optimiser state (frozen template)
                'warp_network': [None] + wp}                       # None = warp_network.progress (no state)

    def group_order(self, cfg_train=None):
        """Optimiser group names in the order the reference builds them for `cfg_train` (any mapping whose keys include the
        `lrate_<name>` entries; None = the merged scan1 configuration).  Groups whose rate is not positive are frozen, not grouped."""
        if cfg_train is None:
            return list(self.GROUPS)
        known = set(self.GROUPS)
        return [k[6:] for k in cfg_train.keys() if k.startswith('lrate_') and k[6:] in known and float(cfg_train[k]) > 0]

    def optimizer_state_dict(self, cfg_train=None):
        c = lambda t: t.detach().clone().cpu().contiguous()
        m, v = self._group_tensors('m'), self._group_tensors('v')
        lr = {'sdf_alpha': self.lr['sdf_ab'], 'sdf_beta': self.lr['sdf_ab'], 'k0': self.lr['k0'], 'rgbnet': self.lr['rgbnet'],
              'warp_network': self.lr['warp'], 'sdf': self.lr['k0']}       # lrate_sdf = lrate_k0 = 0.1 in scan1.py, same decay
        state, groups, idx = {}, [], 0
        for name in self.group_order(cfg_train):
            ids = []
            for tm, tv in zip(m[name], v[name]):
                if tm is not None and self.n_step > 0:
                    state[idx] = {'step': self.n_step, 'exp_avg': c(tm), 'exp_avg_sq': c(tv)}
                ids.append(idx)
                idx += 1
            groups.append({'params': ids, 'lr': float(lr[name]), 'name': name, 'betas': (0.9, 0.99), 'eps': 1e-8,
                           'weight_decay': 0, 'amsgrad': False})
        return {'state': state, 'param_groups': groups}

    def pose_optimizer_state_dict(self):
        c = lambda t: t.detach().clone().cpu()
        state = {0: {'step': self.n_step, 'exp_avg': c(self.se3_m), 'exp_avg_sq': c(self.se3_v)}} if self.n_step > 0 else {}
        return {'state': state, 'param_groups': [{'params': [0], 'lr': float(self.lr_pose), 'betas': (0.9, 0.999), 'eps': 1e-8,
                                                  'weight_decay': 0, 'amsgrad': False}]}

    def load_optimizer_state_dict(self, sd, pose_sd=None):
        """Reads the reference's (or this engine's) torch-Adam layout into the flat moment buffers; groups are matched by
        `name`, parameters by position inside their group.  Groups that are absent keep zero moments."""
        d = lambda t: torch.as_tensor(t, dtype=torch.float32).to(self.dev)
        state = sd['state']
        m, v = self._group_tensors('m'), self._group_tensors('v')
        steps = []
        with torch.no_grad():
            for t in (self.k0_m, self.k0_v, self.flat.m, self.flat.v):
                t.zero_()
            for grp in sd['param_groups']:
                name = grp.get('name')
                if name not in m:
                    continue
                if len(grp['params']) != len(m[name]):
                    raise ValueError(f"optimizer group '{name}': {len(grp['params'])} parameters, expected {len(m[name])}")
                for i, tm, tv in zip(grp['params'], m[name], v[name]):
                    st = state.get(i, state.get(str(i)))
                    if st is None or tm is None:
                        continue
                    tm.copy_(d(st['exp_avg']).reshape(tm.shape))
                    tv.copy_(d(st['exp_avg_sq']).reshape(tv.shape))
                    steps.append(int(st['step']))
                key = {'sdf_alpha': 'sdf_ab', 'sdf_beta': 'sdf_ab', 'warp_network': 'warp'}.get(name, name)
                if key in self.lr:                                 # 'sdf': the frozen template has a group but no rate of ours
                    self.lr[key] = float(grp['lr'])
            if pose_sd is not None and pose_sd.get('state'):
                st = pose_sd['state'].get(0, pose_sd['state'].get('0'))
                self.se3_m.copy_(d(st['exp_avg']))
                self.se3_v.copy_(d(st['exp_avg_sq']))
                self.lr_pose = float(pose_sd['param_groups'][0]['lr'])
        if steps:
            if len(set(steps)) != 1:
                raise ValueError(f'optimizer state with differing step counts {sorted(set(steps))}: the fused Adam keeps one')
            self.n_step = steps[0]

    def load_training_state(self, tensors, se3, se3_m, se3_v, n_step, lr, lr_pose):
        """Resume from an IN-MEMORY training state given in the reference's terms: tensors = {name: (param, exp_avg, exp_avg_sq)}
        with names 'k0' ([1,C,X,Y,Z]), 'sdf_alpha', 'sdf_beta', 'rgbnet.<l>.weight|bias', 'warp.<l>.weight|bias' (logical
        shapes of the reference's modules); lr = {'k0', 'rgbnet', 'warp', 'sdf_ab'}.  Used to put this engine at the state of
        another trainer (teacher-forced parity runs, bench.py); the file-based twin is load_checkpoint."""
        d = lambda t: t.detach().to(self.dev, torch.float32)
        cl = lambda t: d(t)[0].permute(1, 2, 3, 0)
        with torch.no_grad():
            p, m, v = tensors['k0']
            self.k0_cl.copy_(cl(p)); self.k0_m.copy_(cl(m)); self.k0_v.copy_(cl(v))
            F = self.flat
            for which, pick in (('data', 0), ('m', 1), ('v', 2)):
                ab = F.view('sdf_ab', which)
                ab[0:1].copy_(d(tensors['sdf_alpha'][pick]).reshape(1)); ab[1:2].copy_(d(tensors['sdf_beta'][pick]).reshape(1))
                for net in ('rgbnet', 'warp'):
                    for li, (W, b) in enumerate(_unpack(net, F.view(net, which))):
                        W.copy_(d(tensors[f'{net}.{li}.weight'][pick])); b.copy_(d(tensors[f'{net}.{li}.bias'][pick]))
            self.se3.copy_(d(se3)); self.se3_m.copy_(d(se3_m)); self.se3_v.copy_(d(se3_v))
        self.n_step = int(n_step)
        for k in self.lr:
            self.lr[k] = float(lr[k])
        self.lr_pose = float(lr_pose)

    def model_kwargs(self):
        """Constructor arguments of the drop-in `Voxurf` for this engine's configuration, as plain Python values (a checkpoint
        holding them loads weights-only; utils.load_model rebuilds the module from them)."""
        cfg = self.cfg
        rs = [float(cfg.out_range)] * 3
        return {'xyz_min': [float(x) for x in cfg.xyz_min], 'xyz_max': [float(x) for x in cfg.xyz_max],
                'num_voxels': int(cfg.num_voxels), 'num_voxels_base': int(cfg.num_voxels), 'alpha_init': 1e-2,
                'rgbnet_dim': int(cfg.k0_dim), 'rgbnet_direct': True, 'rgbnet_depth': 4, 'rgbnet_width': 128,
                'posbase_pe': int(cfg.posbase_pe), 'viewbase_pe': int(cfg.viewbase_pe), 'geo_rgb_dim': 3,
                's_ratio': float(cfg.s_ratio), 's_start': float(cfg.s_start), 'step_start': float(cfg.step_start),
                'barf_c2f': None if cfg.barf_c2f is None else [float(x) for x in cfg.barf_c2f], 'N_iters': int(cfg.N_iters),
                'i_train': list(range(self.V)), 'HW': [[int(self.H), int(self.W)]] * self.V, 'camera_noise': 0.0,
                'range_shape': rs, 'rect_size': rs}

    def save_checkpoint(self, path, global_step, cfg_train=None):
        """The reference's `last_ckpt.tar` (lib/recon_scene.py:779-791): `global_step`, `current_pose`, `model_kwargs`,
        `MaskCache_kwargs`, `model_state_dict`, `optimizer_state_dict`, `optimizer_pose_state_dict` - the optimiser entries in
        torch-Adam layout - plus this engine's pose parametrisation (`se3_refine`, `w2c_init`) and schedule state."""
        ops.pose_fwd(self.se3, self.w2c_init, self.refine_mask, self.w2c, self.c2w, self.jac)
        c = lambda t: t.detach().clone().cpu()
        cfg = self.cfg
        torch.save({'global_step': int(global_step), 'current_pose': c(self.w2c),
                    'model_kwargs': self.model_kwargs(),
                    'MaskCache_kwargs': {'xyz_min': [float(x) for x in cfg.xyz_min], 'xyz_max': [float(x) for x in cfg.xyz_max],
                                         'act_shift': float(np.log(1 / (1 - 1e-2) - 1)), 'voxel_size_ratio': 1.0, 'nearest': False},
                    'model_state_dict': self.model_state_dict(), 'optimizer_state_dict': self.optimizer_state_dict(cfg_train),
                    'optimizer_pose_state_dict': self.pose_optimizer_state_dict(),
                    'se3_refine': c(self.se3), 'w2c_init': c(self.w2c_init),
                    'engine': {'format': 'poseprobe_amd.TrainEngine/2', 'n_step': self.n_step, 'lr': dict(self.lr),
                               'lr_pose': self.lr_pose}}, path)

    def load_checkpoint(self, path, reload_optimizer=True):
        """-> global_step.  Accepts this engine's files and reference `last_ckpt.tar` files (model under the reference's names,
        optimiser in torch-Adam layout).  Weights-only load (numpy arrays in `model_kwargs` admitted): nothing is executed."""
        from .utils import load_checkpoint_file
        ck = load_checkpoint_file(path)
        self.load_model_state_dict(ck['model_state_dict'])
        d = lambda t: torch.as_tensor(t, dtype=torch.float32).to(self.dev)
        if 'se3_refine' in ck:
            self.se3.copy_(d(ck['se3_refine']))
            self.w2c_init.copy_(d(ck['w2c_init']))
        elif 'current_pose' in ck:                          # a reference file: start from its poses, refinement at zero
            cp = ck['current_pose']
            cp = torch.stack([torch.as_tensor(p) for p in cp]) if isinstance(cp, (list, tuple)) else torch.as_tensor(cp)
            self.w2c_init.copy_(d(cp)[:, :3, :4])
            self.se3.zero_()
        opt = ck.get('optimizer_state_dict', {})
        if reload_optimizer and opt.get('format') == 'poseprobe_amd.TrainEngine/1':     # round-1 files
            self.n_step, self.lr, self.lr_pose = int(opt['n_step']), dict(opt['lr']), float(opt['lr_pose'])
            self.k0_m.copy_(d(opt['k0.exp_avg'])); self.k0_v.copy_(d(opt['k0.exp_avg_sq']))
            self.flat.m.copy_(d(opt['flat.exp_avg'])); self.flat.v.copy_(d(opt['flat.exp_avg_sq']))
            self.se3_m.copy_(d(opt['se3.exp_avg'])); self.se3_v.copy_(d(opt['se3.exp_avg_sq']))
        elif reload_optimizer and 'param_groups' in opt:
            self.load_optimizer_state_dict(opt, ck.get('optimizer_pose_state_dict'))
            eng = ck.get('engine')
            if eng is not None:
                self.n_step, self.lr, self.lr_pose = int(eng['n_step']), dict(eng['lr']), float(eng['lr_pose'])
        self.zero_grads()
        return int(ck.get('global_step', 0))

    def losses(self):
        """dict of the unweighted loss scalars of the last step (one D2H copy)."""
        v = self.ws.loss_out.cpu().numpy()
        names = ['img_render', 'weight_entropy_last', 'grad_constraint', 'grad_deform_constraint',
                 'sdf_correct_constraint', 'sdf_deform_constraint', 'mask_render']
        return {n: float(v[i]) for i, n in enumerate(names)}
